// CPU twin of the kernels of omni-pq_amd/csrc/eval_iou.hip: omni-pq_amd/csrc/obb_iou.h compiled as host C++ (the same
// operations, -ffp-contract=off as in the library's build), run over pairs of boxes from a file.  Built and run by
// tests/test_obb_iou_host_twin.py with AddressSanitizer and UBSan.
//     obb_iou_host_twin IN OUT      IN: int64 n, a8 (n, 8, 3) f64, b8 (n, 8, 3) f64      OUT: (n, 2) f64 = iou3d, iou2d
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "obb_iou.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  long long n = 0;
  if (!f || fread(&n, sizeof n, 1, f) != 1 || n < 0) return 3;
  std::vector<double> a(n * 24), b(n * 24), out(n * 2);
  if (fread(a.data(), sizeof(double), a.size(), f) != a.size() || fread(b.data(), sizeof(double), b.size(), f) != b.size())
    return 3;
  fclose(f);
  for (long long i = 0; i < n; ++i) {
    // a block of exactly the kernels' LDS array, and the slice of its last thread: a vertex written past the two buffers
    // lands outside the allocation, where the sanitizer sees it
    double *lds = (double *)malloc(sizeof(double) * omnipq::kIouRows * omnipq::kIouThreads);
    const omnipq::ObbBox pa = omnipq::load_box(&a[i * 24]), pb = omnipq::load_box(&b[i * 24]);
    omnipq::obb_iou(pa, pb, lds + (omnipq::kIouThreads - 1), out[2 * i], out[2 * i + 1]);
    free(lds);
  }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 4;
  fclose(f);
  return 0;
}
