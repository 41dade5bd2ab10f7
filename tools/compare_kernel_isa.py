#!/usr/bin/env python3
"""Are the kernels of one object file still, instruction for instruction, those of an earlier build?

    python tools/compare_kernel_isa.py OLD.o NEW.o [NAME ...]     exit code 1 and a listing when a kernel of OLD.o differs or is gone
    NAME: compare only the kernels whose name contains one of these strings; a leading `!` excludes instead, e.g.
          '!share_kernel' '!pair_kernel' '!cilqr_solve_kernel<false, 1' '!cilqr_solve_kernel<true, 1' for everything but the kernels that
          run the scalar-path form of the solve's serial loops

Both objects' gfx950 code objects are disassembled (llvm-objdump -d, no raw bytes), addresses and the padding behind the last
s_endpgm dropped, and every kernel of OLD.o compared with its namesake in NEW.o.  A kernel that has since gained a trailing
`false` template argument (a compile-time variant added beside it: warp_kernel -> warp_kernel<false>, warp_batch_kernel<4, false>
-> warp_batch_kernel<4, false, false>) and further parameters is matched with that instantiation.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(obj):
    """{demangled name without its parameter list: [instruction text]} of the device code object inside `obj`."""
    with tempfile.TemporaryDirectory() as d:
        tmp = os.path.join(d, "o.o")
        with open(obj, "rb") as f, open(tmp, "wb") as g:
            g.write(f.read())
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", tmp], cwd=d, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        dev = [os.path.join(d, n) for n in os.listdir(d) if "amdgcn" in n]
        if not dev:
            raise SystemExit("no device code object in %s" % obj)
        text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--demangle", dev[0]], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            cur = out.setdefault(re.sub(r"^void ", "", name[:name.rfind("(")] if "(" in name else name), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//\s*[0-9A-Fa-f]+:.*$", "", line.strip()))
    for body in out.values():  # what follows the last s_endpgm is alignment padding read as instructions
        while body and body[-1] != "s_endpgm":
            body.pop()
    return out


def successors(name):
    """Names an unchanged kernel may carry in the newer object."""
    yield name
    yield name[:-1] + ", false>" if name.endswith(">") else name + "<false>"


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    want = [a for a in sys.argv[3:] if not a.startswith("!")]
    skip = [a[1:] for a in sys.argv[3:] if a.startswith("!")]
    bad = 0
    for name, body in sorted(old.items()):
        if (want and not any(w in name for w in want)) or any(w in name for w in skip):
            continue
        match = next((n for n in successors(name) if n in new), None)
        same = match is not None and new[match] == body
        bad += not same
        print("%-9s %s -> %s (%d instructions)" % ("identical" if same else "DIFFERENT", name, match, len(body)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
