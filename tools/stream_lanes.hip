// stream_lanes.hip -- does a chunk-per-workgroup panel stream with partly filled waves get faster when the same bytes come in
// half as many, twice as wide loads?  (development aid; the probe of profiles/README_paired_panels.md)
//   Kernel kC of stream_widths.hip with only the first m lanes of every wave active, m = 64, 32, 16: a chunk of 0.57 MB per
//   workgroup, 8 workgroups per CU, rows on lanes (4 m rows), four columns per trip.
//     S  4 loads of 8 B in flight per thread, one per column (the panel layout of today)
//     P  2 loads of 16 B in flight per thread, one per column pair (columns 2j, 2j+1 interleaved row by row), 16-byte aligned
//     Q  as P with the chunk starting at an address that is only 8-byte aligned (what a paired panel inside a slab would get)
//   The three forms read the same 8.0 GB with the same lanes and the same bytes in flight; P and Q issue half the vector-memory
//   instructions.  Three repetitions each; the printed spread is max - min of the three.
// Build: hipcc -O3 --offload-arch=gfx950 tools/stream_lanes.hip -o tools/stream_lanes.bin
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <algorithm>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { std::printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

struct __attribute__((aligned(8))) Pair { double a, b; };

// chunk of `len` doubles per workgroup viewed as columns of R = 4 m rows; thread (wave, lane < m) = row wave * m + lane
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) kS(const double* __restrict__ a, int64_t len, int m, double* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane >= m) return;
  const int R = 4 * m;
  const double* p = a + (int64_t)blockIdx.x * len + wave * m + lane;
  const int ncol = (int)(len / R);
  double s[4] = {0, 0, 0, 0};
  for (int k = 0; k + 4 <= ncol; k += 4) {
    double l[4];
#pragma unroll
    for (int u = 0; u < 4; u++) l[u] = p[(int64_t)R * (k + u)];
#pragma unroll
    for (int u = 0; u < 4; u++) s[u] += l[u];
  }
  if (s[0] + s[1] + s[2] + s[3] == 1.2345e300) out[0] = s[0];
}
// the same chunk in column pairs: entry (row, k) at 2 (R j + row) + (k & 1), j = k >> 1
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) kP(const double* __restrict__ a, int64_t len, int m, double* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane >= m) return;
  const int R = 4 * m;
  const double* p = a + (int64_t)blockIdx.x * len + 2 * (wave * m + lane);
  const int npair = (int)(len / R) / 2;
  double s[4] = {0, 0, 0, 0};
  for (int j = 0; j + 2 <= npair; j += 2) {
    Pair l[2];
#pragma unroll
    for (int u = 0; u < 2; u++) l[u] = *reinterpret_cast<const Pair*>(p + (int64_t)2 * R * (j + u));
    s[0] += l[0].a; s[1] += l[0].b; s[2] += l[1].a; s[3] += l[1].b;
  }
  if (s[0] + s[1] + s[2] + s[3] == 1.2345e300) out[0] = s[0];
}

int main() {
  const int64_t nchunk = 13952, len = 71680;          // 0.573 MB per chunk; 8.0 GB in all
  const int64_t n = nchunk * len;
  double *a, *out;
  CK(hipMalloc(&a, (n + 2) * sizeof(double)));
  CK(hipMalloc(&out, 64));
  CK(hipMemset(a, 0, (n + 2) * sizeof(double)));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  std::printf("%-4s %-44s %8s %8s %8s  %8s %7s  %6s\n", "m", "form", "ms", "ms", "ms", "mean", "spread", "TB/s");
  const int ms_[3] = {64, 32, 16};
  for (int mi = 0; mi < 3; mi++) {
    const int m = ms_[mi];
    double mean[3], spread[3];
    const char* names[3] = {"S  4 x 8 B per thread", "P  2 x 16 B per thread, 16-byte aligned", "Q  2 x 16 B per thread, 8-byte aligned"};
    for (int form = 0; form < 3; form++) {
      float t[3];
      for (int rep = -1; rep < 3; rep++) {             // rep -1 warms up
        float ms;
        CK(hipEventRecord(e0));
        if (form == 0) hipLaunchKernelGGL(kS, dim3(nchunk), dim3(256), 0, 0, a, len, m, out);
        else hipLaunchKernelGGL(kP, dim3(nchunk), dim3(256), 0, 0, a + (form == 2 ? 1 : 0), len, m, out);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
        CK(hipGetLastError());
        if (rep >= 0) t[rep] = ms;
      }
      mean[form] = (t[0] + t[1] + t[2]) / 3.0;
      spread[form] = std::max({t[0], t[1], t[2]}) - std::min({t[0], t[1], t[2]});
      std::printf("%-4d %-44s %8.3f %8.3f %8.3f  %8.3f %7.3f  %6.2f\n", m, names[form], t[0], t[1], t[2], mean[form], spread[form], n * 8.0 / mean[form] / 1e9);
    }
    for (int form = 1; form < 3; form++)
      std::printf("%-4d %c against S: %.3f x the time, gain %.3f ms against a spread of %.3f ms\n", m, form == 1 ? 'P' : 'Q', mean[form] / mean[0],
                  mean[0] - mean[form], std::max(spread[0], spread[form]));
  }
  return 0;
}
