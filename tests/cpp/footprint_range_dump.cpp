// footprint_range_dump.cpp — the one place of cilqr_footprint_check where a double becomes a cell index
// (csrc/cilqr_footprint_range.h, compiled here as plain C++), run on the CPU before it ever runs on a device.  Reads cases from
// standard input, one per line:
//     x y theta hl hw  pose_x pose_y pose_theta  x_first y_first res
// (strtod: inf, -inf and nan are accepted) and prints for each
//     ok i_lo i_hi j_lo j_hi  qx0 qy0 qx1 qy1 qx2 qy2 qx3 qy3
// with the corners in the map frame as %.17g.  Heading cosines and sines are the host libm's.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "cilqr_footprint_range.h"

int main() {
  char line[1024];
  while (fgets(line, sizeof(line), stdin)) {
    double v[11];
    char* at = line;
    int n = 0;
    for (; n < 11; ++n) {
      char* end = nullptr;
      v[n] = strtod(at, &end);
      if (end == at) break;
      at = end;
    }
    if (n < 11) continue;
    double qx[4], qy[4];
    cilqr::footprint_corners(v[0], v[1], cos(v[2]), sin(v[2]), v[3], v[4], v[5], v[6], cos(v[7]), sin(v[7]), qx, qy);
    const cilqr::FootprintRange r = cilqr::footprint_range(qx, qy, v[8], v[9], 1.0 / v[10]);
    printf("%d %d %d %d %d", r.ok, r.i_lo, r.i_hi, r.j_lo, r.j_hi);
    for (int k = 0; k < 4; ++k) printf(" %.17g %.17g", qx[k], qy[k]);
    printf("\n");
  }
  return 0;
}
