// edit_harness.hip -- TEST INFRASTRUCTURE, not part of the product library.
// The three verifiers of the edit-distance search (humid_amd/csrc/kernels_graph.hip.h: lev_band1, lev_band2 and
// LevX<0>::dist) on the device on their own, one thread per pair of words, so that tests/test_gpu_edit_sweep.py can
// put them against the plain dynamic programme over every small word and at the word lengths where their code turns
// (1, 2, 31 .. 34, 63, 64).  The pipeline reaches them only through the candidates its joins produce.
// Built by tests/prims_harness.py into tests/_build/ (git-ignored; travels to the GPU box).
#include <hip/hip_runtime.h>

#include "kernels_count.hip.h"      // (block_sum / block_rank, which kernels_graph.hip.h uses, as in pipeline.hip.h)
#include "kernels_graph.hip.h"

namespace {
// out[3 * p + 0 .. 2] = lev_band1, lev_band2, LevX<0> of pair p
template <class WT>
__global__ void __launch_bounds__(256) k_verify(const WT *__restrict__ x, const WT *__restrict__ y, u32 count, u32 n,
                                                u32 *__restrict__ out) {
  HUMID_GUARD_LAST_VGPR();
  const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= count) return;
  const WT wx = x[p], wy = y[p];
  out[3 * p] = lev_band1(wx, wy, n);
  out[3 * p + 1] = lev_band2(wx, wy, n);
  const LevX<0, WT> lx(wx, n);
  out[3 * p + 2] = lx.dist(wy);
}

// host arrays in, host array out; count pairs of n-nucleotide words (n <= 32: one u64 per word, else [hi, lo])
template <class WT>
int verify(const void *hx, const void *hy, u32 count, u32 n, u32 *hout) {
  if (count == 0) return 0;
  WT *dx = nullptr, *dy = nullptr;
  u32 *dout = nullptr;
  int rc = 0;
  const size_t wb = (size_t)count * sizeof(WT), ob = (size_t)count * 3 * sizeof(u32);
  if (hipMalloc((void **)&dx, wb) != hipSuccess || hipMalloc((void **)&dy, wb) != hipSuccess ||
      hipMalloc((void **)&dout, ob) != hipSuccess)
    rc = -1;
  if (!rc && (hipMemcpy(dx, hx, wb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dy, hy, wb, hipMemcpyHostToDevice) != hipSuccess))
    rc = -2;
  if (!rc) {
    hipLaunchKernelGGL(k_verify<WT>, dim3((count + 255) / 256), dim3(256), 0, nullptr, dx, dy, count, n, dout);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = -3;
  }
  if (!rc && hipMemcpy(hout, dout, ob, hipMemcpyDeviceToHost) != hipSuccess) rc = -4;
  if (dx) (void)hipFree(dx);
  if (dy) (void)hipFree(dy);
  if (dout) (void)hipFree(dout);
  return rc;
}
}  // namespace

extern "C" {
int eh_verify(const void *x, const void *y, unsigned count, unsigned word_nt, unsigned *out) {
  if (word_nt < 1 || word_nt > 64) return -10;
  return word_nt <= 32 ? verify<u64>(x, y, count, word_nt, out) : verify<W2>(x, y, count, word_nt, out);
}
}
