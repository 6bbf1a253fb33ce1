// The opening of a cold shared path on an fp32 image of the sample rows (engine_path.hip, "sample start").
//
// The product of the opening's row sample, g = -X_s^T y / n_s, is used for ONE thing: the ranking of |X_j^T y| that chooses
// the first working set.  Nothing is accepted on it (TailArgs::provisional), the model's linear term on W is the exact
// X_W^T y of the gathered fp64 columns, and the first pass over all of X verifies the first band.  A sample entry carries
// sampling noise of sd(y) / sqrt(rows); rounding X to fp32 moves it by 2^-24 relative per term.  So the sample reads a float
// copy of its rows -- half the bytes of a bandwidth-bound pass -- and, since every lane stands at z = 0 without row weights at
// that launch, computes ONE vector instead of the lane slots of the split pass, needs no residual launch in front (R = -y)
// and folds one set of partial sums.  Three kernels:
//   x32_convert_kernel   one read of the fp64 rows, one write of the image; counts what does not survive the conversion
//   sample_xty_kernel    partial[row block][j] = sum_i X32s[i][j] y[i] over the block's rows, fp64 accumulation
//   sample_finish_kernel the row blocks' sums in fixed order, scaled, into the g slot of every lane; the loss into g[ld]
// No floating-point atomics anywhere: the result is the same bits from run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_logic.hpp"  // kSampleThreads, SamplePlan

namespace slm {

// ---------------------------------------------------------------------------------------------
// X32s[i][j] = float(X[i][j]) for i < rows, j < ld32 (ld32 <= ld: the pad columns of X are zero, so are the image's).
// A thread converts four columns of a row: 32 bytes in, 16 out.  *lost counts the entries the image cannot stand in
// for: a finite value that becomes +-inf, and a non-zero value that becomes zero or a subnormal float (which a later
// conversion may flush to zero).  Integer atomics, one per thread that met such an entry.  grid-stride.
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void x32_convert_kernel(const double* __restrict__ X, int64_t rows, int64_t ld, int64_t ld32,
                                                                 float* __restrict__ X32, unsigned int* __restrict__ lost) {
  const int64_t quads = ld32 / 4, total = rows * quads;
  unsigned int bad = 0;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / quads, q = t - i * quads;
    const double2* src = reinterpret_cast<const double2*>(X + i * ld + 4 * q);
    const double2 a = src[0], b = src[1];
    const double v[4] = {a.x, a.y, b.x, b.y};
    float f[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      f[c] = (float)v[c];
      const bool finite = fabs(v[c]) <= 1.7976931348623157e308;  // (false for NaN and +-inf: those convert to themselves)
      if (finite && fabsf(f[c]) > 3.4028234663852886e38f) ++bad;
      if (v[c] != 0.0 && fabsf(f[c]) < 1.1754943508222875e-38f) ++bad;
    }
    *reinterpret_cast<float4*>(X32 + i * ld32 + 4 * q) = make_float4(f[0], f[1], f[2], f[3]);
  }
  if (bad) atomicAdd(lost, bad);
}

struct SampleArgs {
  const float* X32;   // [n_s][ld32]
  const double* y;    // [n_s]
  double* partial;    // [yb][pstride] the sums of every column over a row block; then [yb] the blocks' sums of y^2
  double* g;          // [n_lanes][ld + 16]
  const int* done;    // nullable; *done != 0: the solve is over, return at once
  int64_t n_s, ld32, ld, rows, pstride;
  int p, yb, n_lanes;
  double scale;       // 1 / n_eff of the sample
};

// ---------------------------------------------------------------------------------------------
// grid (column blocks of 4 * kSampleThreads columns, row blocks of a.rows rows), kSampleThreads threads.  A thread owns
// four columns and walks ALL rows of its row block: one 16-byte load per row, U of them in flight, widened to double in
// registers and multiplied by y[i] (the same address in every lane: a scalar load) on the vector units -- four FMAs per
// 16 bytes, far below the vector rate at this bandwidth.  The sums leave as two 16-byte stores.  No LDS, no barrier.
// ---------------------------------------------------------------------------------------------
template <int U>
static __global__ __launch_bounds__(slm_host::kSampleThreads) void sample_xty_kernel(SampleArgs a) {
  if (a.done != nullptr && *a.done != 0) return;
  const int64_t col = ((int64_t)blockIdx.x * slm_host::kSampleThreads + threadIdx.x) * 4;
  if (col >= a.ld32) return;
  const int64_t i0 = (int64_t)blockIdx.y * a.rows;
  const int64_t i1 = i0 + a.rows < a.n_s ? i0 + a.rows : a.n_s;
  const float* __restrict__ x = a.X32 + col;
  const double* __restrict__ y = a.y;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  double yy = 0.0;
  int64_t i = i0;
  for (; i + U <= i1; i += U) {
    float4 v[U];
    double yv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v[u] = *reinterpret_cast<const float4*>(x + (i + u) * a.ld32);
      yv[u] = y[i + u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      acc[0] = __builtin_fma((double)v[u].x, yv[u], acc[0]);
      acc[1] = __builtin_fma((double)v[u].y, yv[u], acc[1]);
      acc[2] = __builtin_fma((double)v[u].z, yv[u], acc[2]);
      acc[3] = __builtin_fma((double)v[u].w, yv[u], acc[3]);
      yy = __builtin_fma(yv[u], yv[u], yy);
    }
  }
  for (; i < i1; ++i) {
    const float4 v = *reinterpret_cast<const float4*>(x + i * a.ld32);
    const double yi = y[i];
    acc[0] = __builtin_fma((double)v.x, yi, acc[0]);
    acc[1] = __builtin_fma((double)v.y, yi, acc[1]);
    acc[2] = __builtin_fma((double)v.z, yi, acc[2]);
    acc[3] = __builtin_fma((double)v.w, yi, acc[3]);
    yy = __builtin_fma(yi, yi, yy);
  }
  double2* out = reinterpret_cast<double2*>(a.partial + (int64_t)blockIdx.y * a.pstride + col);
  out[0] = make_double2(acc[0], acc[1]);
  out[1] = make_double2(acc[2], acc[3]);
  if (col == 0) a.partial[(int64_t)a.yb * a.pstride + blockIdx.y] = yy;  // (every thread of the row block holds the same sum)
}

// ---------------------------------------------------------------------------------------------
// grid (ld / 16 + 1), 256 threads = 16 columns x 16 slices, as reduce_partials_kernel: slice s adds the row blocks s, s + 16,
// ... of its column in that order, the sixteen slices are added in order, and g[lane][j] = -scale * sum goes to EVERY lane of
// the call (they all stand at zero).  The trailing workgroup does the same for the blocks' sums of y^2: g[lane][ld] =
// scale / 2 * sum, the loss at zero on the sample.  Columns from p on are written as zeros.
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void sample_finish_kernel(SampleArgs a) {
  if (a.done != nullptr && *a.done != 0) return;
  __shared__ double lds[16][17];
  const int tid = threadIdx.x;
  const int cl = tid & 15, slice = tid >> 4;
  const int64_t col = (int64_t)blockIdx.x * 16 + cl;
  const bool loss_block = (int64_t)blockIdx.x * 16 >= a.ld;
  double s = 0.0;
  if (!loss_block) {
    if (col < a.ld32)
      for (int b = slice; b < a.yb; b += 16) s += a.partial[(int64_t)b * a.pstride + col];
  } else {
    for (int b = tid; b < a.yb; b += 256) s += a.partial[(int64_t)a.yb * a.pstride + b];
  }
  lds[slice][cl] = s;
  __syncthreads();
  if (!loss_block) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += lds[k][cl];
    const double v = col < a.p ? -(t * a.scale) : 0.0;
    for (int lane = slice; lane < a.n_lanes; lane += 16) a.g[(int64_t)lane * (a.ld + 16) + col] = v;
  } else {
    double t = 0.0;
    for (int k = 0; k < 16; ++k)
      for (int c = 0; c < 16; ++c) t += lds[k][c];
    const double v = t * (0.5 * a.scale);
    for (int lane = tid; lane < a.n_lanes; lane += 256) a.g[(int64_t)lane * (a.ld + 16) + a.ld] = v;
  }
}

}  // namespace slm
