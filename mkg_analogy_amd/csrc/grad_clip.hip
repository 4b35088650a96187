// Gradient clipping / gradient-norm tracking over the flat gradient buffer (include/mart_clip.h): three streaming kernels beside the fused
// AdamW step (head_optim.hip), driven by the same chunk table.  HBM-bound: 16-byte accesses, double accumulation for free.
#include "common.h"
#include "mart_clip.h"

#include <limits.h>

namespace {
constexpr int TPB = 256;
constexpr int CLIP_PART = 8192;                 // elements per piece: 8 x 16 bytes per lane, as adamw_k's parts
constexpr int CLIP_PARTS = MART_CLIP_PARTS;     // work items per chunk (a 65536-element chunk: one piece each)
constexpr int CLIP_GRID = 2048;                 // 256 CUs x 8 four-wave workgroups; more work items than that are swept in a grid-stride loop
constexpr int ZERO_ONLY = 4;                    // chunk flag bit 2 (mart_adamw_desc.chunks)

// max that a NaN on either side survives (fmax drops it)
__device__ __forceinline__ double nan_max(double a, double b) { return (a != a || a > b) ? a : b; }

template <int MODE> __device__ __forceinline__ double fold(double acc, float x) {
  if (MODE == MART_CLIP_NORM_2) { const double d = (double)x; return acc + d * d; }
  return nan_max(acc, (double)__builtin_fabsf(x));
}
template <int MODE> __device__ __forceinline__ double combine(double a, double b) { return MODE == MART_CLIP_NORM_2 ? a + b : nan_max(a, b); }

// the workgroup's value from its 256 lanes, in a fixed order (xor butterfly inside a wave, then the four waves in turn); valid in every lane.
// Ends with a barrier, so ``red`` can be reused right away.
template <int MODE> __device__ __forceinline__ double block_combine(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = combine<MODE>(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = red[0];
#pragma unroll
  for (int w = 1; w < TPB / 64; ++w) r = combine<MODE>(r, red[w]);
  __syncthreads();
  return r;
}

// Every element of work item ``part`` of the chunk [start, start + len), each exactly once: ``v4`` on the 16-byte aligned quads, ``s1`` on the up
// to three single elements at either end of a piece (chunk starts are not multiples of 4: adaptive_weight spans, odd-sized biases).
template <class P, class V4, class S1> __device__ __forceinline__ void for_part(P* g, int start, int len, int part, V4 v4, S1 s1) {
  for (int base = part * CLIP_PART; base < len; base += CLIP_PARTS * CLIP_PART) {
    const int n = min(CLIP_PART, len - base);
    P* p = g + (long long)start + base;
    const int head = min(n, (int)((4u - (unsigned)(((uintptr_t)p >> 2) & 3u)) & 3u));
    const int nv = (n - head) >> 2, tail0 = head + 4 * nv;
    if ((int)threadIdx.x < head) s1(p + threadIdx.x);
#pragma unroll 4
    for (int k = threadIdx.x; k < nv; k += TPB) v4(p + head + 4 * k);
    if ((int)threadIdx.x < n - tail0) s1(p + tail0 + threadIdx.x);
  }
}

template <int MODE> __global__ __launch_bounds__(TPB) void clip_sumsq_k(const float* grad, const int32_t* chunks, int n_chunks, double* partials, int n_partials) {
  __shared__ double red[TPB / 64];
  const int n_items = n_chunks * CLIP_PARTS;
  for (int wi = blockIdx.x; wi < n_partials; wi += gridDim.x) {
    double acc = 0.0;
    if (wi < n_items) {
      const int ci = wi / CLIP_PARTS, part = wi % CLIP_PARTS;
      const int start = chunks[3 * ci], len = chunks[3 * ci + 1], flags = chunks[3 * ci + 2];
      if (!(flags & ZERO_ONLY))
        for_part(grad, start, len, part,
                 [&](const float* q) {
                   const f32x4 x = *(const f32x4*)q;
#pragma unroll
                   for (int e = 0; e < 4; ++e) acc = fold<MODE>(acc, x[e]);
                 },
                 [&](const float* q) { acc = fold<MODE>(acc, *q); });
    }
    const double r = block_combine<MODE>(acc, red);
    if (threadIdx.x == 0) partials[wi] = r;
  }
}

__global__ __launch_bounds__(TPB) void clip_finalize_k(const double* partials, int n_partials, int mode, float grad_scale, float max_norm, float* out,
                                                       float* log, int log_index) {
  __shared__ double red[TPB / 64];
  double acc = 0.0;
  if (mode == MART_CLIP_NORM_2)
    for (int i = threadIdx.x; i < n_partials; i += TPB) acc += partials[i];
  else
    for (int i = threadIdx.x; i < n_partials; i += TPB) acc = nan_max(acc, partials[i]);
  const double s = mode == MART_CLIP_NORM_2 ? block_combine<MART_CLIP_NORM_2>(acc, red) : block_combine<MART_CLIP_NORM_INF>(acc, red);
  if (threadIdx.x == 0) {
    const float total = (float)((double)grad_scale * (mode == MART_CLIP_NORM_2 ? sqrt(s) : s));
    float coef = 1.0f;
    if (max_norm > 0.f) {
      // torch.nn.utils.clip_grad_norm_'s ``max_norm / (total_norm + 1e-6)`` as torch evaluates it on an fp32 tensor: scalar / tensor is
      // tensor.reciprocal() * scalar (Tensor.__rtruediv__), i.e. two roundings -- one division would differ in the last bit on a quarter of the inputs
      coef = (1.0f / (total + 1e-6f)) * max_norm;
      coef = coef > 1.0f ? 1.0f : coef;           // clamp(max=1): a NaN compares false and stays
    }
    out[0] = total;
    out[1] = coef;
    if (log) log[log_index] = total;
  }
}

__global__ __launch_bounds__(TPB) void clip_apply_k(float* grad, const int32_t* chunks, int n_chunks, const float* coef_ptr, float clip_value) {
  const bool by_value = clip_value > 0.f;
  const float coef = by_value ? 1.0f : *coef_ptr;
  if (!by_value && coef == 1.0f) return;          // the clip did not trigger: wave-uniform, nothing is read or written
  const float lo = -clip_value, hi = clip_value;
  auto f = [&](float x) { return by_value ? (x < lo ? lo : (x > hi ? hi : x)) : x * coef; };   // NaN: both comparisons false, stays NaN
  const int n_items = n_chunks * CLIP_PARTS;
  for (int wi = blockIdx.x; wi < n_items; wi += gridDim.x) {
    const int ci = wi / CLIP_PARTS, part = wi % CLIP_PARTS;
    const int start = chunks[3 * ci], len = chunks[3 * ci + 1], flags = chunks[3 * ci + 2];
    if (flags & ZERO_ONLY) continue;
    for_part(grad, start, len, part,
             [&](float* q) {
               f32x4 x = *(f32x4*)q;
#pragma unroll
               for (int e = 0; e < 4; ++e) x[e] = f(x[e]);
               *(f32x4*)q = x;
             },
             [&](float* q) { *q = f(*q); });
  }
}

int grid_for(long long items) { return items < CLIP_GRID ? (int)items : CLIP_GRID; }
}  // namespace

extern "C" int mart_clip_partials_needed(int n_chunks) {
  MART_CHECK(n_chunks > 0 && n_chunks <= INT_MAX / CLIP_PARTS, "clip_partials_needed: n_chunks out of range");
  return n_chunks * CLIP_PARTS;
}
extern "C" int mart_clip_sumsq(const float* grad, const int32_t* chunks, int n_chunks, int mode, double* partials, int n_partials, void* stream) {
  MART_CHECK(grad && chunks && partials, "clip_sumsq: null pointer");
  MART_CHECK(n_chunks > 0 && n_chunks <= INT_MAX / CLIP_PARTS, "clip_sumsq: n_chunks out of range");
  MART_CHECK(mode == MART_CLIP_NORM_2 || mode == MART_CLIP_NORM_INF, "clip_sumsq: unknown mode (0: 2-norm, 1: inf-norm)");
  MART_CHECK(n_partials >= n_chunks * CLIP_PARTS, "clip_sumsq: n_partials is smaller than mart_clip_partials_needed(n_chunks)");
  const int g = grid_for(n_partials);
  if (mode == MART_CLIP_NORM_2)
    hipLaunchKernelGGL(clip_sumsq_k<MART_CLIP_NORM_2>, dim3(g), dim3(TPB), 0, (hipStream_t)stream, grad, chunks, n_chunks, partials, n_partials);
  else
    hipLaunchKernelGGL(clip_sumsq_k<MART_CLIP_NORM_INF>, dim3(g), dim3(TPB), 0, (hipStream_t)stream, grad, chunks, n_chunks, partials, n_partials);
  MART_LAUNCH_CHECK();
  return 0;
}
extern "C" int mart_clip_finalize(const double* partials, int n_partials, int mode, float grad_scale, float max_norm, float* out, float* log,
                                  int log_index, void* stream) {
  MART_CHECK(partials && out, "clip_finalize: null pointer");
  MART_CHECK(n_partials > 0, "clip_finalize: n_partials must be positive");
  MART_CHECK(mode == MART_CLIP_NORM_2 || mode == MART_CLIP_NORM_INF, "clip_finalize: unknown mode (0: 2-norm, 1: inf-norm)");
  MART_CHECK(log_index >= 0, "clip_finalize: negative log_index");
  hipLaunchKernelGGL(clip_finalize_k, dim3(1), dim3(TPB), 0, (hipStream_t)stream, partials, n_partials, mode, grad_scale, max_norm, out, log, log_index);
  MART_LAUNCH_CHECK();
  return 0;
}
extern "C" int mart_clip_apply(float* grad, const int32_t* chunks, int n_chunks, const float* coef_ptr, float clip_value, void* stream) {
  MART_CHECK(grad && chunks, "clip_apply: null pointer");
  MART_CHECK(clip_value > 0.f || coef_ptr, "clip_apply: norm mode (clip_value <= 0) needs coef_ptr");
  MART_CHECK(n_chunks > 0 && n_chunks <= INT_MAX / CLIP_PARTS, "clip_apply: n_chunks out of range");
  hipLaunchKernelGGL(clip_apply_k, dim3(grid_for((long long)n_chunks * CLIP_PARTS)), dim3(TPB), 0, (hipStream_t)stream, grad, chunks, n_chunks, coef_ptr,
                     clip_value);
  MART_LAUNCH_CHECK();
  return 0;
}
