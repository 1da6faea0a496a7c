// krylov_hip.hip -- HIP (gfx950 / MI355X) kernels of the native Krylov solver (krylov.hpp, krylov.cpp).
//
// One ICGS(2) step w <- (I - V V^T)^2 w over k basis columns (column-major, one contiguous column per Krylov vector)
// reads the basis three times from HBM:
//   k_kry_tile<false>   pass A: h1 = V^T w.  A workgroup stages a tile of 64 rows x k columns in LDS (each wave reads
//                       512 contiguous bytes of one column) and thread j accumulates column j's dot over all tiles of
//                       its grid stride in a register: one partial per workgroup and column
//   k_kry_tile<true>    pass B: the same tile first gives w - V h1 for its 64 rows (four quarter sums per row, added in
//                       a fixed order), then the dots of the new w with the tile that is still in LDS: h2 = V^T w
//   k_kry_rows<true>    pass C: dst = w - V h2, one row per thread, k coalesced column reads; the norm partials of dst
//   k_kry_rows<false>   x += V y (solution update), the same kernel without the norm
//   k_kry_reduce*       stage two of every reduction: the partials of one column summed by one workgroup in a fixed
//                       tree, on the device, so h1 feeds pass B and h2 pass C without a host round trip
//   k_kry_border_*      the border product of a bordered system [K V; W' C] behind K x: y += V s and the tail W' x + C s
//   k_kry_proj_*        projection vectors: y = x - P (G (Q' x)), the coefficients in two stages and one update pass
//   k_kry_shifted       the shifted operator y = a K x + b B x: both CSR matrices in one pass, y written once
// plus the vector passes of GMRES and CG.  No atomics anywhere: every result is bitwise reproducible.
//
// Every pass is written once, as a __device__ body (kry_*_body, kry_column_sum); a __global__ kernel only finds its operands
// and calls the body.  The single-column kernel passes its arguments and its launch grid, the lock-step kernel (_mv) the
// operands of column blockIdx.y and that column's own grid: one text, so a batched column cannot drift from its single launch.
//
// k_kry_tile and k_kry_rows take the element type of the basis.  With float ("MI Basis Storage" = single) a basis entry
// is widened when it is used and every product and sum stays FP64; the tile in LDS holds floats (column stride 65
// floats, krylov.hpp: kry_tile_lds_f32), which is what bounds the workgroups per CU of passes A and B.  Three small
// kernels go with it: k_kry_widen (the FP64 copy of a column), k_kry_round_div and k_kry_round_scale_by (a quotient
// formed in FP64 and rounded once into a float column).
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include <type_traits>
#include "krylov.hpp"

namespace hymls {
namespace dev {

#define KRY_CHECK(call)                                                                    \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess)                                                                  \
      throw ::hymls::Error(-3, std::string("HIP error: ") + hipGetErrorString(e_) + " at " + \
                                   __FILE__ + ":" + std::to_string(__LINE__));             \
  } while (0)

static inline hipStream_t kstream() { return (hipStream_t)stream(); }
static inline int vec_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, KRY_MAXGRID)); }

// fixed-order sum of the 256 values of red[] (every thread holds one; result in red[0])
__device__ inline void block_sum256(double* red) {
  for (int st = 128; st > 0; st >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
  }
  __syncthreads();
}
// block_sum256 for MC columns at once (results in red[j][0])
template <int MC>
__device__ inline void block_sum256_cols(double (*red)[256]) {
  const int t = threadIdx.x;
  for (int st = 128; st > 0; st >>= 1) {
    __syncthreads();
    if (t < st) {
#pragma unroll
      for (int j = 0; j < MC; j++) red[j][t] += red[j][t + st];
    }
  }
  __syncthreads();
}
// stage two of every reduction: the sum of the nb stage-one partials part[b * stride + j] of column j, each thread its
// partials b = t, t + 256, .. in ascending order, then the fixed tree.  The result is valid on thread 0 alone (only that
// thread reads red[0], so a caller may go straight on to the next column)
__device__ inline double kry_column_sum(const double* __restrict__ part, int nb, int64_t stride, int j, double* red) {
  const int t = threadIdx.x;
  double s = 0.0;
  for (int b = t; b < nb; b += 256) s += part[(int64_t)b * stride + j];
  red[t] = s;
  block_sum256(red);
  return t == 0 ? red[0] : 0.0;
}
// element c of a per-column table that travels as an int4 kernel argument
__device__ inline int kry_pick(int4 v, int c) { return c == 0 ? v.x : (c == 1 ? v.y : (c == 2 ? v.z : v.w)); }

// ---- passes A and B; BT: the element type of the basis (double, or float with "MI Basis Storage" = single).  Every product
// and sum is FP64: a float entry is widened when it leaves LDS.  own: the workgroups that walk the tiles of this column
// (unsigned, as gridDim.x is: the tile index then advances by the same instructions in both callers)
template <bool UPD, class BT>
__device__ __forceinline__ void kry_tile_body(int64_t n, int k, const BT* __restrict__ V, int64_t ldv, double* w,
                                              const double* __restrict__ h1, double* __restrict__ part, unsigned own) {
  extern __shared__ double sm[];
  constexpr bool F32 = sizeof(BT) == 4;
  constexpr int T = KRY_TILE, LT = F32 ? KRY_LD_TILE_F32 : KRY_LD_TILE;
  // FP64 basis: tile, ws, hs, red.  FP32 basis: the FP64 arrays first, so that they stay 8-byte aligned for every k
  BT* Vs = F32 ? (BT*)(sm + T + KRY_KMAX + 4 * T) : (BT*)sm;   // [k][LT]: column j of the tile at Vs[j * LT]
  double* ws = F32 ? sm : sm + (size_t)LT * k;                 // [T]
  double* hs = ws + T;               // [KRY_KMAX]
  double* red = hs + KRY_KMAX;       // [4][T]
  const int t = threadIdx.x;
  if (UPD)
    for (int j = t; j < k; j += 256) hs[j] = h1[j];
  double acc = 0.0;
  const int64_t ntiles = (n + T - 1) / T;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += own) {
    const int64_t r0 = tile * T;
    const int rows = (int)(n - r0 < T ? n - r0 : T);
    __syncthreads();   // the previous tile is no longer read
    for (int e = t; e < T * k; e += 256) {
      const int r = e & (T - 1), j = e / T;
      Vs[j * LT + r] = r < rows ? V[(int64_t)j * ldv + r0 + r] : (BT)0;
    }
    if (t < T) ws[t] = t < rows ? w[r0 + t] : 0.0;
    __syncthreads();
    if (UPD) {
      // w - V h1 for the tile: wave q adds the columns j = q mod 4 of row r = lane, the four sums are added in wave order
      const int r = t & (T - 1), q = t / T;
      double s = 0.0;
      for (int j = q; j < k; j += 4) s += (double)Vs[j * LT + r] * hs[j];
      red[q * T + r] = s;
      __syncthreads();
      if (t < T) {
        const double v = ws[t] - (((red[t] + red[T + t]) + red[2 * T + t]) + red[3 * T + t]);
        ws[t] = v;   // rows past n: 0 - 0
        if (t < rows) w[r0 + t] = v;
      }
      __syncthreads();
    }
    if (t < k) {
      const BT* c = Vs + t * LT;
#pragma unroll 8
      for (int r = 0; r < T; r++) acc += (double)c[r] * ws[r];
    }
  }
  if (t < k) part[(int64_t)blockIdx.x * k + t] = acc;
}
template <bool UPD, class BT>
__global__ void __launch_bounds__(256) k_kry_tile(int64_t n, int k, const BT* __restrict__ V, int64_t ldv, double* w,
                                                  const double* __restrict__ h1, double* __restrict__ part) {
  kry_tile_body<UPD, BT>(n, k, V, ldv, w, h1, part, gridDim.x);
}

// ---- pass C (NORM) and the solution update; the launch grid is the column's own grid (kry_row_grid(n))
template <bool NORM, class BT>
__device__ __forceinline__ void kry_rows_body(int64_t n, int k, const BT* __restrict__ V, int64_t ldv,
                                              const double* __restrict__ h, const double* w, double* dst,
                                              double* __restrict__ part) {
  __shared__ double hs[KRY_KMAX];
  __shared__ double red[256];
  const int t = threadIdx.x;
  for (int j = t; j < k; j += 256) hs[j] = h[j];
  __syncthreads();
  double ss = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + t; i < n; i += (int64_t)gridDim.x * 256) {
    const BT* v = V + i;
    double s = 0.0;
#pragma unroll 8
    for (int j = 0; j < k; j++) s += (double)v[(int64_t)j * ldv] * hs[j];
    if (NORM) {
      const double x = w[i] - s;
      dst[i] = x;
      ss += x * x;
    } else {
      dst[i] = w[i] + s;
    }
  }
  if (NORM) {
    red[t] = ss;
    block_sum256(red);
    if (t == 0) part[blockIdx.x] = red[0];
  }
}
template <bool NORM, class BT>
__global__ void __launch_bounds__(256) k_kry_rows(int64_t n, int k, const BT* __restrict__ V, int64_t ldv,
                                                  const double* __restrict__ h, const double* w, double* dst,
                                                  double* __restrict__ part) {
  kry_rows_body<NORM, BT>(n, k, V, ldv, h, w, dst, part);
}

// ---- stage two: dst[j] = sum over the nb partials of column j (and dst2[j] = add[j] + dst[j])
__global__ void __launch_bounds__(256) k_kry_reduce(const double* __restrict__ part, int nb, int k, double* dst,
                                                    const double* add, double* dst2) {
  __shared__ double red[256];
  const int j = blockIdx.x;
  const double s = kry_column_sum(part, nb, k, j, red);
  if (threadIdx.x == 0) {
    dst[j] = s;
    if (add) dst2[j] = add[j] + s;
  }
}
// dst[0] = sqrt(s), dst[1] = s
__global__ void __launch_bounds__(256) k_kry_reduce_norm(const double* __restrict__ part, int nb, double* dst) {
  __shared__ double red[256];
  const double s = kry_column_sum(part, nb, 1, 0, red);
  if (threadIdx.x == 0) { dst[0] = std::sqrt(s); dst[1] = s; }
}

// ---- vector passes; a body strides by the launch grid, which is vec_grid(n) for one column and for a batch
__device__ __forceinline__ void kry_scale_by_body(int64_t n, double* x, const double* d) {
  const double s = *d;
  if (!(s > 0.0)) return;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) x[i] = x[i] / s;
}
__device__ __forceinline__ void kry_widen_body(int64_t n, const float* __restrict__ v, double* __restrict__ t) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) t[i] = (double)v[i];
}
__device__ __forceinline__ void kry_round_scale_by_body(int64_t n, const double* __restrict__ x, const double* d,
                                                        float* __restrict__ y) {
  const double s = *d;
  const bool pos = s > 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    y[i] = (float)(pos ? x[i] / s : x[i]);
}
__device__ __forceinline__ void kry_dot_body(int64_t n, const double* __restrict__ x, const double* __restrict__ y,
                                             double* __restrict__ part) {
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) s += x[i] * y[i];
  red[threadIdx.x] = s;
  block_sum256(red);
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
__device__ __forceinline__ void kry_cg_xr_body(int64_t n, double alpha, const double* __restrict__ p,
                                               const double* __restrict__ q, double* __restrict__ x,
                                               double* __restrict__ r, double* __restrict__ part) {
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    x[i] = x[i] + alpha * p[i];
    const double v = r[i] - alpha * q[i];
    r[i] = v;
    s += v * v;
  }
  red[threadIdx.x] = s;
  block_sum256(red);
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
__device__ __forceinline__ void kry_cg_p_body(int64_t n, double beta, const double* __restrict__ z, double* __restrict__ p) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = z[i] + beta * p[i];
}

__global__ void __launch_bounds__(256) k_kry_scale_by(int64_t n, double* x, const double* d) { kry_scale_by_body(n, x, d); }
__global__ void __launch_bounds__(256) k_kry_div(int64_t n, const double* x, double s, double* y) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = x[i] / s;
}
// FP32 basis: the widening copy of a column, and the two stores that round a quotient formed in FP64 once
__global__ void __launch_bounds__(256) k_kry_widen(int64_t n, const float* __restrict__ v, double* __restrict__ t) {
  kry_widen_body(n, v, t);
}
__global__ void __launch_bounds__(256) k_kry_round_div(int64_t n, const double* __restrict__ x, double s, float* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = (float)(x[i] / s);
}
__global__ void __launch_bounds__(256) k_kry_round_scale_by(int64_t n, const double* __restrict__ x, const double* d,
                                                            float* __restrict__ y) {
  kry_round_scale_by_body(n, x, d, y);
}
__global__ void __launch_bounds__(256) k_kry_sub(int64_t n, const double* b, const double* y, double* r) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) r[i] = b[i] - y[i];
}
__global__ void __launch_bounds__(256) k_kry_add(int64_t n, const double* x, double* y) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = y[i] + x[i];
}
__global__ void __launch_bounds__(256) k_kry_dot(int64_t n, const double* __restrict__ x, const double* __restrict__ y,
                                                 double* __restrict__ part) {
  kry_dot_body(n, x, y, part);
}
__global__ void __launch_bounds__(256) k_kry_cg_xr(int64_t n, double alpha, const double* __restrict__ p,
                                                   const double* __restrict__ q, double* __restrict__ x,
                                                   double* __restrict__ r, double* __restrict__ part) {
  kry_cg_xr_body(n, alpha, p, q, x, r, part);
}
__global__ void __launch_bounds__(256) k_kry_cg_p(int64_t n, double beta, const double* __restrict__ z, double* __restrict__ p) {
  kry_cg_p_body(n, beta, z, p);
}

// ---- bordered operator (krylov.hpp: kry_border_product).  Stage one, MC <= KRY_BORDER_CHUNK columns [c0, c0 + MC) of the
// border: one row per thread, the MC coalesced column reads of V and of W; y[i] += sum_j V[i, j] s_j (j ascending) and the
// thread's partials of W(:, j)' x in registers, summed per workgroup in the fixed tree into part[workgroup * m + c0 + j]
template <int MC>
__global__ void __launch_bounds__(256) k_kry_border_rows(int64_t n, int m, int c0, const double* __restrict__ V, int64_t ldv,
                                                         const double* __restrict__ W, int64_t ldw,
                                                         const double* __restrict__ z, double* __restrict__ y,
                                                         double* __restrict__ part) {
  __shared__ double red[MC][256];
  const int t = threadIdx.x;
  const double* Vc = V + (int64_t)c0 * ldv;
  const double* Wc = W + (int64_t)c0 * ldw;
  double s[MC], acc[MC];
#pragma unroll
  for (int j = 0; j < MC; j++) { s[j] = z[n + c0 + j]; acc[j] = 0.0; }   // the border scalars: the tail of z, on the device
  for (int64_t i = (int64_t)blockIdx.x * 256 + t; i < n; i += (int64_t)gridDim.x * 256) {
    const double xi = z[i];
    double sv = 0.0;
#pragma unroll
    for (int j = 0; j < MC; j++) {
      sv += Vc[(int64_t)j * ldv + i] * s[j];
      acc[j] += Wc[(int64_t)j * ldw + i] * xi;
    }
    y[i] = y[i] + sv;
  }
#pragma unroll
  for (int j = 0; j < MC; j++) red[j][t] = acc[j];
  block_sum256_cols<MC>(red);
  if (t < MC) part[(int64_t)blockIdx.x * m + c0 + t] = red[t][0];
}
// stage two, one workgroup: y[n + j] = (the nb partials of column j, summed as k_kry_reduce does) + sum_l C[j + m l] s_l
__global__ void __launch_bounds__(256) k_kry_border_tail(const double* __restrict__ part, int nb, int64_t n, int m,
                                                         const double* __restrict__ dC, const double* __restrict__ z,
                                                         double* __restrict__ y) {
  __shared__ double red[256];
  for (int j = 0; j < m; j++) {
    double v = kry_column_sum(part, nb, m, j, red);
    if (threadIdx.x == 0) {
      if (dC)
        for (int l = 0; l < m; l++) v += dC[j + (int64_t)m * l] * z[n + l];
      y[n + j] = v;
    }
  }
}

// ---- projection vectors (krylov.hpp: kry_oblique_project), y = x - P (G (Q' x)).  Stage one of the coefficients, MC <=
// KRY_PROJ_CHUNK columns [c0, c0 + MC) of Q: one row per thread, the MC column reads coalesced across the wave, the thread's
// partials of Q(:, j)' x in registers, summed per workgroup in the fixed tree into part[workgroup * m + c0 + j]
template <int MC>
__global__ void __launch_bounds__(256) k_kry_proj_dots(int64_t n, int m, int c0, const double* __restrict__ Q, int64_t ldq,
                                                       const double* __restrict__ x, double* __restrict__ part) {
  __shared__ double red[MC][256];
  const int t = threadIdx.x;
  const double* Qc = Q + (int64_t)c0 * ldq;
  double acc[MC];
#pragma unroll
  for (int j = 0; j < MC; j++) acc[j] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + t; i < n; i += (int64_t)gridDim.x * 256) {
    const double xi = x[i];
#pragma unroll
    for (int j = 0; j < MC; j++) acc[j] += Qc[(int64_t)j * ldq + i] * xi;
  }
#pragma unroll
  for (int j = 0; j < MC; j++) red[j][t] = acc[j];
  block_sum256_cols<MC>(red);
  if (t < MC) part[(int64_t)blockIdx.x * m + c0 + t] = red[t][0];
}
// stage two, one workgroup: c_j = the nb partials of column j, summed as k_kry_reduce does; then thread j forms
// d_j = sum_l G[j + m l] c_l with l ascending (d = c without G)
__global__ void __launch_bounds__(256) k_kry_proj_tail(const double* __restrict__ part, int nb, int m,
                                                       const double* __restrict__ dG, double* __restrict__ d) {
  __shared__ double red[256];
  __shared__ double cs[KRY_PROJ_MAX];
  const int t = threadIdx.x;
  for (int j = 0; j < m; j++) {
    const double c = kry_column_sum(part, nb, m, j, red);
    if (t == 0) cs[j] = c;
  }
  __syncthreads();
  if (t < m) {
    double v = cs[t];
    if (dG) {
      v = 0.0;
      for (int l = 0; l < m; l++) v += dG[t + (int64_t)m * l] * cs[l];
    }
    d[t] = v;
  }
}
// y_i = x_i - sum_j P[i, j] d_j: one pass over the rows for every m, the coefficients once per workgroup in LDS (every lane
// reads the same address: a broadcast), the m column reads coalesced across the wave.  y may be x: a thread reads x_i
// before it writes y_i and touches no other row
__global__ void __launch_bounds__(256) k_kry_proj_update(int64_t n, int m, const double* __restrict__ P, int64_t ldp,
                                                         const double* __restrict__ d, const double* x, double* y) {
  __shared__ double ds[KRY_PROJ_MAX];
  const int t = threadIdx.x;
  if (t < m) ds[t] = d[t];
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + t; i < n; i += (int64_t)gridDim.x * 256) {
    const double* p = P + i;
    double s = 0.0;
#pragma unroll 8
    for (int j = 0; j < m; j++) s += p[(int64_t)j * ldp] * ds[j];
    y[i] = x[i] - s;
  }
}

// ---- shifted operator (krylov.hpp: kry_shifted_product): Y(:, v) = a A X(:, v) + b B X(:, v) for NV columns in one pass.
// The L lanes of a row keep two sums per column, over the row of A and over the row of B, each formed as k_spmv<L>
// (device_hip.hip) forms its sum: entries rp[row] + lane, step L, ascending, then the __shfl_down tree.  A lane loads each
// (col, val) pair once for all NV columns.  a == 0, b == 0 and rpB == nullptr are uniform over the launch, so every lane of
// a sub-wave takes the same branches and takes part in the shuffles; the trip count of the grid-stride loop is uniform inside
// a workgroup for the same reason as in k_spmv.  One body for every L and NV: the single-vector form is NV = 1.
template <int L, int NV>
__global__ void __launch_bounds__(256) k_kry_shifted(int32_t n, const int32_t* __restrict__ rpA, const int32_t* __restrict__ colA,
                                                     const double* __restrict__ valA, const int32_t* __restrict__ rpB,
                                                     const int32_t* __restrict__ colB, const double* __restrict__ valB, double a,
                                                     double b, const double* __restrict__ x, int64_t ldx, double* __restrict__ y,
                                                     int64_t ldy) {
  const int lane = (int)(threadIdx.x % L);
  const int rpb = (int)blockDim.x / L;   // rows per block and pass
  const bool useA = a != 0.0, useB = b != 0.0, haveB = rpB != nullptr;
  for (int64_t base = (int64_t)blockIdx.x * rpb; base < n; base += (int64_t)gridDim.x * rpb) {
    const int64_t row = base + threadIdx.x / L;
    double sA[NV], sB[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) sA[v] = sB[v] = 0.0;
    if (row < n) {
      if (useA) {
        const int e = rpA[row + 1];
        for (int k = rpA[row] + lane; k < e; k += L) {
          const double av = valA[k];
          const int64_t c = colA[k];
#pragma unroll
          for (int v = 0; v < NV; v++) sA[v] += av * x[c + v * ldx];
        }
      }
      if (useB && haveB) {
        const int e = rpB[row + 1];
        for (int k = rpB[row] + lane; k < e; k += L) {
          const double bv = valB[k];
          const int64_t c = colB[k];
#pragma unroll
          for (int v = 0; v < NV; v++) sB[v] += bv * x[c + v * ldx];
        }
      } else if (useB && lane == 0) {   // the identity: the row sum is x[row] itself
#pragma unroll
        for (int v = 0; v < NV; v++) sB[v] = x[row + v * ldx];
      }
    }
#pragma unroll
    for (int v = 0; v < NV; v++) {
      if (useA) {
#pragma unroll
        for (int off = L / 2; off > 0; off >>= 1) sA[v] += __shfl_down(sA[v], off, L);
      }
      if (useB && haveB) {
#pragma unroll
        for (int off = L / 2; off > 0; off >>= 1) sB[v] += __shfl_down(sB[v], off, L);
      }
      if (row < n && lane == 0) y[row + v * ldy] = !useB ? a * sA[v] : (!useA ? b * sB[v] : a * sA[v] + b * sB[v]);
    }
  }
}

// ---- lock-step columns (krylov.hpp: KryBatch, KryVecBatch): blockIdx.y is the column.  Each kernel calls the body of its
// single-column kernel above with the operands of its column and the column's own grid: a column strides by the grid its
// single-column launch would have had and writes that many partials, so its sums are added in the same order and give the
// same bits whatever the other columns of the launch are.  Passes A and B: the own grid is `own`, and workgroups past it
// leave before the first barrier.  Every other pass: the own grid is the same for all columns and is the launch grid.
template <bool UPD, class BT>
__global__ void __launch_bounds__(256) k_kry_tile_mv(int64_t n, int64_t ldv, KryBatch B, int4 owns) {
  const int c = blockIdx.y;
  const int own = kry_pick(owns, c);   // kry_tile_grid[_f32](n, k) of this column
  if ((int)blockIdx.x >= own) return;
  kry_tile_body<UPD, BT>(n, B.k[c], (const BT*)B.V[c], ldv, B.w[c], B.ws[c].h1, B.ws[c].part, own);
}
// pass C of the batch
template <class BT>
__global__ void __launch_bounds__(256) k_kry_rows_mv(int64_t n, int64_t ldv, KryBatch B) {
  const int c = blockIdx.y;
  kry_rows_body<true, BT>(n, B.k[c], (const BT*)B.V[c], ldv, B.ws[c].h2, B.w[c], B.dst[c], B.ws[c].part);
}

// stage two of passes A (UPD false: h1) and B (h2, out = h1 + h2): grid (largest k, columns); nbs[c]: the partials of column c
template <bool UPD>
__global__ void __launch_bounds__(256) k_kry_reduce_mv(KryBatch B, int4 nbs) {
  __shared__ double red[256];
  const int c = blockIdx.y, j = blockIdx.x;
  const int k = B.k[c];
  if (j >= k) return;
  const double s = kry_column_sum(B.ws[c].part, kry_pick(nbs, c), k, j, red);
  if (threadIdx.x == 0) {
    if (UPD) { B.ws[c].h2[j] = s; B.ws[c].out[j] = B.ws[c].h1[j] + s; }
    else B.ws[c].h1[j] = s;
  }
}
__global__ void __launch_bounds__(256) k_kry_reduce_norm_mv(KryBatch B, int nb) {
  __shared__ double red[256];
  const int c = blockIdx.y;
  double* dst = B.ws[c].out + B.k[c];
  const double s = kry_column_sum(B.ws[c].part, nb, 1, 0, red);
  if (threadIdx.x == 0) { dst[0] = std::sqrt(s); dst[1] = s; }
}
// stage two of the batched dots: out[c][0] = the sum of the nb partials of column c (k_kry_reduce with k = 1)
__global__ void __launch_bounds__(256) k_kry_reduce1_mv(KryVecBatch B, int nb) {
  __shared__ double red[256];
  const int c = blockIdx.y;
  const double s = kry_column_sum(B.part[c], nb, 1, 0, red);
  if (threadIdx.x == 0) B.out[c][0] = s;
}

__global__ void __launch_bounds__(256) k_kry_scale_by_mv(int64_t n, KryVecBatch B) {
  const int c = blockIdx.y;
  kry_scale_by_body(n, (double*)B.y[c], B.d[c]);
}
__global__ void __launch_bounds__(256) k_kry_widen_mv(int64_t n, KryVecBatch B) {
  const int c = blockIdx.y;
  kry_widen_body(n, (const float*)B.a[c], (double*)B.y[c]);
}
__global__ void __launch_bounds__(256) k_kry_round_scale_by_mv(int64_t n, KryVecBatch B) {
  const int c = blockIdx.y;
  kry_round_scale_by_body(n, (const double*)B.a[c], B.d[c], (float*)B.y[c]);
}
__global__ void __launch_bounds__(256) k_kry_dot_mv(int64_t n, KryVecBatch B) {
  const int c = blockIdx.y;
  kry_dot_body(n, (const double*)B.a[c], B.b[c], B.part[c]);
}
__global__ void __launch_bounds__(256) k_kry_cg_xr_mv(int64_t n, KryVecBatch B) {
  const int c = blockIdx.y;
  kry_cg_xr_body(n, B.s[c], (const double*)B.a[c], B.b[c], (double*)B.y[c], B.r[c], B.part[c]);
}
__global__ void __launch_bounds__(256) k_kry_cg_p_mv(int64_t n, KryVecBatch B) {
  const int c = blockIdx.y;
  kry_cg_p_body(n, B.s[c], (const double*)B.a[c], (double*)B.y[c]);
}

static inline void kcheck() { KRY_CHECK(hipGetLastError()); }

// lets the two tile kernels of one basis type (passes A and B; F32: a float tile) use the LDS of KRY_KMAX columns.  The
// attribute is per device: attr_device is the caller's record of the device that has it (one variable per kernel pair)
static void allow_tile_lds(const void* pass_a, const void* pass_b, bool F32, int& attr_device) {
  int devno = 0;
  KRY_CHECK(hipGetDevice(&devno));
  if (attr_device == devno) return;
  const int most = (int)(F32 ? kry_tile_lds_f32(KRY_KMAX) : kry_tile_lds(KRY_KMAX));
  KRY_CHECK(hipFuncSetAttribute(pass_a, hipFuncAttributeMaxDynamicSharedMemorySize, most));
  KRY_CHECK(hipFuncSetAttribute(pass_b, hipFuncAttributeMaxDynamicSharedMemorySize, most));
  attr_device = devno;
}
// f(std::integral_constant<int, mc>()) for a chunk of mc = 1..8 columns: the launch of a kernel that has MC as a template parameter
static_assert(KRY_BORDER_CHUNK == 8 && KRY_PROJ_CHUNK == 8, "for_chunk_width dispatches 1..8 columns");
template <class F>
static void for_chunk_width(int mc, F&& f) {
  switch (mc) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    case 5: f(std::integral_constant<int, 5>()); break;
    case 6: f(std::integral_constant<int, 6>()); break;
    case 7: f(std::integral_constant<int, 7>()); break;
    default: f(std::integral_constant<int, 8>()); break;
  }
}

template <bool UPD, class BT>
static void tile_pass(int64_t n, int32_t k, const BT* V, int64_t ldv, double* w, const KryWork& ws) {
  if (k < 1 || k > KRY_KMAX) throw Error(-2, "orthogonalisation: 1 <= k <= 256 columns");
  constexpr bool F32 = sizeof(BT) == 4;
  const int nb = F32 ? kry_tile_grid_f32(n, k) : kry_tile_grid(n, k);
  const size_t shm = F32 ? kry_tile_lds_f32(k) : kry_tile_lds(k);
  static thread_local int attr_device = -1;
  allow_tile_lds((const void*)k_kry_tile<false, BT>, (const void*)k_kry_tile<true, BT>, F32, attr_device);
  hipLaunchKernelGGL((k_kry_tile<UPD, BT>), dim3(nb), dim3(256), shm, kstream(), n, k, V, ldv, w, ws.h1, ws.part);
  kcheck();
  if (UPD) hipLaunchKernelGGL(k_kry_reduce, dim3(k), dim3(256), 0, kstream(), ws.part, nb, k, ws.h2, ws.h1, ws.out);
  else hipLaunchKernelGGL(k_kry_reduce, dim3(k), dim3(256), 0, kstream(), ws.part, nb, k, ws.h1, nullptr, nullptr);
  kcheck();
}
template <class BT>
static void row_pass_c(int64_t n, int32_t k, const BT* V, int64_t ldv, const double* w, double* dst, const KryWork& ws) {
  if (k < 1 || k > KRY_KMAX) throw Error(-2, "orthogonalisation: 1 <= k <= 256 columns");
  const int nb = kry_row_grid(n);
  hipLaunchKernelGGL((k_kry_rows<true, BT>), dim3(nb), dim3(256), 0, kstream(), n, k, V, ldv, ws.h2, w, dst, ws.part);
  kcheck();
  hipLaunchKernelGGL(k_kry_reduce_norm, dim3(1), dim3(256), 0, kstream(), ws.part, nb, ws.out + k);
  kcheck();
}
template <class BT>
static void row_update(int64_t n, int32_t k, const BT* V, int64_t ldv, const double* y, double* x) {
  if (k < 1) return;
  if (k > KRY_KMAX) throw Error(-2, "basis update: at most 256 columns");
  hipLaunchKernelGGL((k_kry_rows<false, BT>), dim3(kry_row_grid(n)), dim3(256), 0, kstream(), n, k, V, ldv, y, x, x, nullptr);
  kcheck();
}

void kry_pass_a(int64_t n, int32_t k, const double* V, int64_t ldv, const double* w, const KryWork& ws) {
  tile_pass<false>(n, k, V, ldv, const_cast<double*>(w), ws);
}
void kry_pass_b(int64_t n, int32_t k, const double* V, int64_t ldv, double* w, const KryWork& ws) {
  tile_pass<true>(n, k, V, ldv, w, ws);
}
void kry_pass_c(int64_t n, int32_t k, const double* V, int64_t ldv, const double* w, double* dst, const KryWork& ws) {
  row_pass_c(n, k, V, ldv, w, dst, ws);
}
void kry_update(int64_t n, int32_t k, const double* V, int64_t ldv, const double* y, double* x) {
  row_update(n, k, V, ldv, y, x);
}
void kry_pass_a(int64_t n, int32_t k, const float* V, int64_t ldv, const double* w, const KryWork& ws) {
  tile_pass<false>(n, k, V, ldv, const_cast<double*>(w), ws);
}
void kry_pass_b(int64_t n, int32_t k, const float* V, int64_t ldv, double* w, const KryWork& ws) {
  tile_pass<true>(n, k, V, ldv, w, ws);
}
void kry_pass_c(int64_t n, int32_t k, const float* V, int64_t ldv, const double* w, double* dst, const KryWork& ws) {
  row_pass_c(n, k, V, ldv, w, dst, ws);
}
void kry_update(int64_t n, int32_t k, const float* V, int64_t ldv, const double* y, double* x) {
  row_update(n, k, V, ldv, y, x);
}
void kry_widen(int64_t n, const float* v, double* t) {
  hipLaunchKernelGGL(k_kry_widen, dim3(vec_grid(n)), dim3(256), 0, kstream(), n, v, t);
  kcheck();
}
void kry_round_div(int64_t n, const double* x, double s, float* y) {
  hipLaunchKernelGGL(k_kry_round_div, dim3(vec_grid(n)), dim3(256), 0, kstream(), n, x, s, y);
  kcheck();
}
void kry_round_scale_by(int64_t n, const double* x, const double* d, float* y) {
  hipLaunchKernelGGL(k_kry_round_scale_by, dim3(vec_grid(n)), dim3(256), 0, kstream(), n, x, d, y);
  kcheck();
}
void kry_scale_by(int64_t n, double* x, const double* d) {
  hipLaunchKernelGGL(k_kry_scale_by, dim3(vec_grid(n)), dim3(256), 0, kstream(), n, x, d);
  kcheck();
}
void kry_div(int64_t n, const double* x, double s, double* y) {
  hipLaunchKernelGGL(k_kry_div, dim3(vec_grid(n)), dim3(256), 0, kstream(), n, x, s, y);
  kcheck();
}
void kry_sub(int64_t n, const double* b, const double* y, double* r) {
  hipLaunchKernelGGL(k_kry_sub, dim3(vec_grid(n)), dim3(256), 0, kstream(), n, b, y, r);
  kcheck();
}
void kry_add(int64_t n, const double* x, double* y) {
  hipLaunchKernelGGL(k_kry_add, dim3(vec_grid(n)), dim3(256), 0, kstream(), n, x, y);
  kcheck();
}
void kry_dot(int64_t n, const double* x, const double* y, const KryWork& ws) {
  const int nb = vec_grid(n);
  hipLaunchKernelGGL(k_kry_dot, dim3(nb), dim3(256), 0, kstream(), n, x, y, ws.part);
  kcheck();
  hipLaunchKernelGGL(k_kry_reduce, dim3(1), dim3(256), 0, kstream(), ws.part, nb, 1, ws.out, nullptr, nullptr);
  kcheck();
}
void kry_cg_xr(int64_t n, double alpha, const double* p, const double* q, double* x, double* r, const KryWork& ws) {
  const int nb = vec_grid(n);
  hipLaunchKernelGGL(k_kry_cg_xr, dim3(nb), dim3(256), 0, kstream(), n, alpha, p, q, x, r, ws.part);
  kcheck();
  hipLaunchKernelGGL(k_kry_reduce, dim3(1), dim3(256), 0, kstream(), ws.part, nb, 1, ws.out, nullptr, nullptr);
  kcheck();
}
void kry_cg_p(int64_t n, double beta, const double* z, double* p) {
  hipLaunchKernelGGL(k_kry_cg_p, dim3(vec_grid(n)), dim3(256), 0, kstream(), n, beta, z, p);
  kcheck();
}

void kry_border_product(int64_t n, int32_t m, const double* V, int64_t ldv, const double* W, int64_t ldw, const double* dC,
                        const double* z, double* y, const KryWork& ws) {
  if (n < 1 || m < 1 || m > KRY_BORDER_MAX || ldv < n || ldw < n) throw Error(-2, "border product: n >= 1, 1 <= m <= 32, ldv, ldw >= n");
  const int nb = kry_row_grid(n);
  for (int c0 = 0; c0 < m; c0 += KRY_BORDER_CHUNK)
    for_chunk_width(std::min(KRY_BORDER_CHUNK, m - c0), [&](auto mc) {
      hipLaunchKernelGGL((k_kry_border_rows<decltype(mc)::value>), dim3(nb), dim3(256), 0, kstream(), n, m, c0, V, ldv, W, ldw, z,
                         y, ws.part);
      kcheck();
    });
  hipLaunchKernelGGL(k_kry_border_tail, dim3(1), dim3(256), 0, kstream(), ws.part, nb, n, m, dC, z, y);
  kcheck();
}

void kry_proj_coeffs(int64_t n, int32_t m, const double* Q, int64_t ldq, const double* dG, const double* x, const KryWork& ws) {
  if (n < 1 || m < 1 || m > KRY_PROJ_MAX || ldq < n) throw Error(-2, "oblique projection: n >= 1, 1 <= m <= 32, ldq >= n");
  const int nb = kry_row_grid(n);
  for (int c0 = 0; c0 < m; c0 += KRY_PROJ_CHUNK)
    for_chunk_width(std::min(KRY_PROJ_CHUNK, m - c0), [&](auto mc) {
      hipLaunchKernelGGL((k_kry_proj_dots<decltype(mc)::value>), dim3(nb), dim3(256), 0, kstream(), n, m, c0, Q, ldq, x, ws.part);
      kcheck();
    });
  hipLaunchKernelGGL(k_kry_proj_tail, dim3(1), dim3(256), 0, kstream(), ws.part, nb, m, dG, ws.h1);
  kcheck();
}
void kry_proj_update(int64_t n, int32_t m, const double* P, int64_t ldp, const double* x, double* y, const KryWork& ws) {
  if (n < 1 || m < 1 || m > KRY_PROJ_MAX || ldp < n) throw Error(-2, "oblique projection: n >= 1, 1 <= m <= 32, ldp >= n");
  hipLaunchKernelGGL(k_kry_proj_update, dim3(kry_row_grid(n)), dim3(256), 0, kstream(), n, m, P, ldp, ws.h1, x, y);
  kcheck();
}
void kry_oblique_project(int64_t n, int32_t m, const double* Q, int64_t ldq, const double* dG, const double* P, int64_t ldp,
                         const double* x, double* y, const KryWork& ws) {
  if (ldp < n) throw Error(-2, "oblique projection: n >= 1, 1 <= m <= 32, ldp >= n");   // before the first launch
  kry_proj_coeffs(n, m, Q, ldq, dG, x, ws);
  kry_proj_update(n, m, P, ldp, x, y, ws);
}

template <int L>
static void shifted_launch(int nv, dim3 grid, int32_t n, const int32_t* rpA, const int32_t* colA, const double* valA, const int32_t* rpB,
                           const int32_t* colB, const double* valB, double a, double b, const double* x, int64_t ldx, double* y,
                           int64_t ldy) {
  switch (nv) {
    case 1: hipLaunchKernelGGL((k_kry_shifted<L, 1>), grid, dim3(256), 0, kstream(), n, rpA, colA, valA, rpB, colB, valB, a, b, x, ldx, y, ldy); break;
    case 2: hipLaunchKernelGGL((k_kry_shifted<L, 2>), grid, dim3(256), 0, kstream(), n, rpA, colA, valA, rpB, colB, valB, a, b, x, ldx, y, ldy); break;
    case 3: hipLaunchKernelGGL((k_kry_shifted<L, 3>), grid, dim3(256), 0, kstream(), n, rpA, colA, valA, rpB, colB, valB, a, b, x, ldx, y, ldy); break;
    default: hipLaunchKernelGGL((k_kry_shifted<L, 4>), grid, dim3(256), 0, kstream(), n, rpA, colA, valA, rpB, colB, valB, a, b, x, ldx, y, ldy); break;
  }
  kcheck();
}
void kry_shifted_product(int32_t n, const int32_t* rpA, const int32_t* colA, const double* valA, int64_t nnzA_hint,
                         const int32_t* rpB, const int32_t* colB, const double* valB, double a, double b, const double* X,
                         int64_t ldx, double* Y, int64_t ldy, int nv) {
  if (n < 1 || nv < 0 || ldx < n || ldy < n || !X || !Y || (a != 0.0 && (!rpA || !colA || !valA)) || (rpB && (!colB || !valB)))
    throw Error(-2, "shifted product: n >= 1, nv >= 0, ldx, ldy >= n, non-null X, Y and arrays of A (unless a = 0)");
  const int L = spmv_lanes(n, nnzA_hint);
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(((int64_t)n * L + 255) / 256, 1 << 20)));   // the grid of spmv()
  for (int v0 = 0; v0 < nv; v0 += 4) {
    const int g = std::min(4, nv - v0);
    const double* xg = X + (int64_t)v0 * ldx;
    double* yg = Y + (int64_t)v0 * ldy;
    switch (L) {
      case 1: shifted_launch<1>(g, grid, n, rpA, colA, valA, rpB, colB, valB, a, b, xg, ldx, yg, ldy); break;
      case 2: shifted_launch<2>(g, grid, n, rpA, colA, valA, rpB, colB, valB, a, b, xg, ldx, yg, ldy); break;
      case 4: shifted_launch<4>(g, grid, n, rpA, colA, valA, rpB, colB, valB, a, b, xg, ldx, yg, ldy); break;
      default: shifted_launch<8>(g, grid, n, rpA, colA, valA, rpB, colB, valB, a, b, xg, ldx, yg, ldy); break;
    }
  }
}

// ---- lock-step launchers
static void check_batch(const KryBatch& b) {
  if (b.nb < 1 || b.nb > KRY_LOCKSTEP_MAX) throw Error(-2, "batched orthogonalisation: 1 <= columns <= 4");
  for (int c = 0; c < b.nb; c++)
    if (b.k[c] < 1 || b.k[c] > KRY_KMAX) throw Error(-2, "orthogonalisation: 1 <= k <= 256 columns");
}
template <bool UPD, class BT>
static void tile_pass_mv(int64_t n, int64_t ldv, const KryBatch& b) {
  check_batch(b);
  constexpr bool F32 = sizeof(BT) == 4;
  int own[KRY_LOCKSTEP_MAX] = {0, 0, 0, 0};
  int grid = 1, kmax = 1;
  size_t shm = 0;
  for (int c = 0; c < b.nb; c++) {
    own[c] = F32 ? kry_tile_grid_f32(n, b.k[c]) : kry_tile_grid(n, b.k[c]);
    grid = std::max(grid, own[c]);
    kmax = std::max(kmax, (int)b.k[c]);
    shm = std::max(shm, F32 ? kry_tile_lds_f32(b.k[c]) : kry_tile_lds(b.k[c]));
  }
  static thread_local int attr_device = -1;
  allow_tile_lds((const void*)k_kry_tile_mv<false, BT>, (const void*)k_kry_tile_mv<true, BT>, F32, attr_device);
  const int4 owns = make_int4(own[0], own[1], own[2], own[3]);
  hipLaunchKernelGGL((k_kry_tile_mv<UPD, BT>), dim3(grid, b.nb), dim3(256), shm, kstream(), n, ldv, b, owns);
  kcheck();
  hipLaunchKernelGGL(k_kry_reduce_mv<UPD>, dim3(kmax, b.nb), dim3(256), 0, kstream(), b, owns);
  kcheck();
}
void kry_pass_a_mv(int64_t n, int64_t ldv, const KryBatch& b, bool f32) {
  if (f32) tile_pass_mv<false, float>(n, ldv, b); else tile_pass_mv<false, double>(n, ldv, b);
}
void kry_pass_b_mv(int64_t n, int64_t ldv, const KryBatch& b, bool f32) {
  if (f32) tile_pass_mv<true, float>(n, ldv, b); else tile_pass_mv<true, double>(n, ldv, b);
}
void kry_pass_c_mv(int64_t n, int64_t ldv, const KryBatch& b, bool f32) {
  check_batch(b);
  const int nb = kry_row_grid(n);
  if (f32) hipLaunchKernelGGL(k_kry_rows_mv<float>, dim3(nb, b.nb), dim3(256), 0, kstream(), n, ldv, b);
  else hipLaunchKernelGGL(k_kry_rows_mv<double>, dim3(nb, b.nb), dim3(256), 0, kstream(), n, ldv, b);
  kcheck();
  hipLaunchKernelGGL(k_kry_reduce_norm_mv, dim3(1, b.nb), dim3(256), 0, kstream(), b, nb);
  kcheck();
}
static void check_vec_batch(const KryVecBatch& b) {
  if (b.nb < 1 || b.nb > KRY_LOCKSTEP_MAX) throw Error(-2, "batched vector pass: 1 <= columns <= 4");
}
void kry_scale_by_mv(int64_t n, const KryVecBatch& b) {
  check_vec_batch(b);
  hipLaunchKernelGGL(k_kry_scale_by_mv, dim3(vec_grid(n), b.nb), dim3(256), 0, kstream(), n, b);
  kcheck();
}
void kry_round_scale_by_mv(int64_t n, const KryVecBatch& b) {
  check_vec_batch(b);
  hipLaunchKernelGGL(k_kry_round_scale_by_mv, dim3(vec_grid(n), b.nb), dim3(256), 0, kstream(), n, b);
  kcheck();
}
void kry_widen_mv(int64_t n, const KryVecBatch& b) {
  check_vec_batch(b);
  hipLaunchKernelGGL(k_kry_widen_mv, dim3(vec_grid(n), b.nb), dim3(256), 0, kstream(), n, b);
  kcheck();
}
void kry_dot_mv(int64_t n, const KryVecBatch& b) {
  check_vec_batch(b);
  const int nb = vec_grid(n);
  hipLaunchKernelGGL(k_kry_dot_mv, dim3(nb, b.nb), dim3(256), 0, kstream(), n, b);
  kcheck();
  hipLaunchKernelGGL(k_kry_reduce1_mv, dim3(1, b.nb), dim3(256), 0, kstream(), b, nb);
  kcheck();
}
void kry_cg_xr_mv(int64_t n, const KryVecBatch& b) {
  check_vec_batch(b);
  const int nb = vec_grid(n);
  hipLaunchKernelGGL(k_kry_cg_xr_mv, dim3(nb, b.nb), dim3(256), 0, kstream(), n, b);
  kcheck();
  hipLaunchKernelGGL(k_kry_reduce1_mv, dim3(1, b.nb), dim3(256), 0, kstream(), b, nb);
  kcheck();
}
void kry_cg_p_mv(int64_t n, const KryVecBatch& b) {
  check_vec_batch(b);
  hipLaunchKernelGGL(k_kry_cg_p_mv, dim3(vec_grid(n), b.nb), dim3(256), 0, kstream(), n, b);
  kcheck();
}

// ---- phase timing
struct KryTimer {
  struct Rec { int phase; bool begin; hipEvent_t ev; };
  std::vector<Rec> log;
  std::vector<hipEvent_t> pool;
};
KryTimer* kry_timer_create() { return new KryTimer(); }
void kry_timer_destroy(KryTimer* t) {
  if (!t) return;
  for (auto& r : t->log) (void)hipEventDestroy(r.ev);
  for (auto e : t->pool) (void)hipEventDestroy(e);
  delete t;
}
void kry_mark(KryTimer* t, int phase, bool begin) {
  hipEvent_t e;
  if (!t->pool.empty()) { e = t->pool.back(); t->pool.pop_back(); }
  else KRY_CHECK(hipEventCreate(&e));
  KRY_CHECK(hipEventRecord(e, kstream()));
  t->log.push_back({phase, begin, e});
}
void kry_collect(KryTimer* t, double* sum) {
  KRY_CHECK(hipStreamSynchronize(kstream()));
  hipEvent_t open[4] = {};
  for (auto& r : t->log) {
    if (r.begin) open[r.phase] = r.ev;
    else if (open[r.phase]) {
      float ms = 0;
      KRY_CHECK(hipEventElapsedTime(&ms, open[r.phase], r.ev));
      sum[r.phase] += 1e-3 * ms;
    }
  }
  for (auto& r : t->log) t->pool.push_back(r.ev);
  t->log.clear();
}

}  // namespace dev
}  // namespace hymls
