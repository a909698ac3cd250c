// Parameter-sized work of one optimisation step as THREE launches over flat buffers (the
// reference leaves it to Lightning: torch.optim.Adam(betas=(0.5, 0.999)) + gradient_clip_val 0.25 under native AMP,
// /root/reference/gloria/builder.py:84-87, run.py:172-207):
//   glr_sumsq_partial   per-workgroup sums of squares of a flat gradient buffer (bf16 or fp32), fixed order
//   glr_clip_coef       total norm over all partials -> { norm, min(1, max_norm / (norm + 1e-6)) } on the device
//                       (torch.nn.utils.clip_grad_norm_'s coefficient, no host round trip)
//   glr_adam_step       Adam (torch semantics: L2 weight decay added to the gradient, bias corrections) on the fp32
//                       MASTER weights with the clipped gradient, writing the bf16 SHADOW the forward reads in the
//                       same pass: no per-step autocast weight casts, no gradient casts, one launch per dtype group
//                       instead of ~600 small kernels.  HBM-bound: 4 + 4 + 4 + 2 read, 4 + 4 + 4 + 2 written per
//                       shadowed parameter.
// Guarded forms (the `GUARD` instantiations, glr_*_g): the sums of squares also count the non-finite gradient elements
// of their share and note the first one, glr_step_guard turns that into a per-step skip decision in a small device
// record (include/glr.h GLR_GUARD_*), and the Adam kernels return without writing anything when the step is skipped -
// GradScaler's skip of native AMP, decided on the device with no host round trip.  The unguarded instantiations are
// the code of the plain entry points, unchanged.
#include <climits>
#include <cmath>

#include "glr_common.h"

namespace {

constexpr int OPT_NT = 256;
constexpr int OPT_VEC = 8;          // elements per thread per trip

__device__ __forceinline__ void load8(const void* p, int dtype, size_t i, float (&v)[8]) {
  if (dtype == GLR_BF16) {
    const uint4 u = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(p) + i);
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[2 * k] = __uint_as_float(w[k] << 16);
      v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
    }
  } else {
    const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + i);
    const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + i + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
}

// inf / NaN test on the exponent bits (a bf16 value widened to fp32 keeps them: (u & 0x7f80) == 0x7f80 in bf16)
__device__ __forceinline__ bool non_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// a thread's count of non-finite elements and the smallest offset among them
struct BadSeen {
  long long n = 0, first = LLONG_MAX;
  __device__ __forceinline__ void see(float x, long long off) {
    if (non_finite(x)) { ++n; first = off < first ? off : first; }
  }
};

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ long long wave_min_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const long long u = __shfl_xor(v, o, 64); v = u < v ? u : v; }
  return v;
}

// nf[2 b] = non-finite count of block b's share, nf[2 b + 1] = the smallest offset among them (-1: none).  No atomics:
// every workgroup owns its two slots, like partial[b].
__device__ __forceinline__ void write_bad(BadSeen bad, long long* __restrict__ nf) {
  __shared__ long long rn[OPT_NT / 64], rf[OPT_NT / 64];
  bad.n = wave_sum_ll(bad.n);
  bad.first = wave_min_ll(bad.first);
  if ((threadIdx.x & 63) == 0) { rn[threadIdx.x >> 6] = bad.n; rf[threadIdx.x >> 6] = bad.first; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long n = (rn[0] + rn[1]) + (rn[2] + rn[3]);
    long long f = rf[0] < rf[1] ? rf[0] : rf[1];
    f = rf[2] < f ? rf[2] : f;
    f = rf[3] < f ? rf[3] : f;
    nf[2 * (size_t)blockIdx.x] = n;
    nf[2 * (size_t)blockIdx.x + 1] = n ? f : -1;
  }
}

// partial[blockIdx.x] = sum of squares of this block's contiguous share (n is a multiple of 8: buffers are padded);
// GUARD: + its non-finite count and first non-finite offset in x
template <bool GUARD>
__global__ void __launch_bounds__(OPT_NT) k_sumsq(const void* __restrict__ x, int dtype, size_t n, float* __restrict__ partial,
                                                  long long* __restrict__ nf) {
  __shared__ float red[OPT_NT / 64];
  const size_t per = ((n / OPT_VEC + gridDim.x - 1) / gridDim.x) * OPT_VEC;
  const size_t lo = (size_t)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
  float s = 0.f;
  BadSeen bad;
  for (size_t i = lo + (size_t)threadIdx.x * OPT_VEC; i < hi; i += (size_t)OPT_NT * OPT_VEC) {
    float v[8];
    load8(x, dtype, i, v);
#pragma unroll
    for (int k = 0; k < 8; ++k) s = __builtin_fmaf(v[k], v[k], s);
    if constexpr (GUARD) {
#pragma unroll
      for (int k = 0; k < 8; ++k) bad.see(v[k], (long long)(i + k));
    }
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  if constexpr (GUARD) write_bad(bad, nf);
}

// out[0] = sqrt(sum partial), out[1] = clip coefficient (1 when max_norm <= 0)
__global__ void __launch_bounds__(OPT_NT) k_clip_coef(const float* __restrict__ partial, int n, float max_norm,
                                                      float* __restrict__ out) {
  __shared__ float red[OPT_NT / 64];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += OPT_NT) s += partial[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float norm = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
    out[0] = norm;
    out[1] = max_norm > 0.f ? fminf(1.f, max_norm / (norm + 1e-6f)) : 1.f;
  }
}

// out[0] = sqrt(sum partial), out[1] = the coefficient - the arithmetic of k_clip_coef, in the same order - and the
// step's skip decision in rec (include/glr.h GLR_GUARD_*): skipped when ANY element counted by the guarded sums of
// squares is inf / NaN (GradScaler's test).  Finite elements whose norm overflows are not skipped: coefficient 0 as in
// k_clip_coef.  One workgroup; thread 0 updates the record.
__global__ void __launch_bounds__(OPT_NT) k_step_guard(const float* __restrict__ partial, const long long* __restrict__ nf,
                                                       int n, float max_norm, float* __restrict__ out,
                                                       long long* __restrict__ rec, long long call) {
  __shared__ float red[OPT_NT / 64];
  __shared__ long long rn[OPT_NT / 64], rf[OPT_NT / 64];
  float s = 0.f;
  long long cnt = 0, first = LLONG_MAX;          // first: the smallest partial index with a non-finite element
  for (int i = threadIdx.x; i < n; i += OPT_NT) {
    s += partial[i];
    const long long c = nf[2 * (size_t)i];
    cnt += c;
    if (c != 0 && i < first) first = i;
  }
  s = wave_sum(s);
  cnt = wave_sum_ll(cnt);
  first = wave_min_ll(first);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = s; rn[threadIdx.x >> 6] = cnt; rf[threadIdx.x >> 6] = first; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float norm = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
    out[0] = norm;
    out[1] = max_norm > 0.f ? fminf(1.f, max_norm / (norm + 1e-6f)) : 1.f;
    const long long bad = (rn[0] + rn[1]) + (rn[2] + rn[3]);
    if (bad == 0) {
      rec[GLR_GUARD_APPLIED] += 1;
      rec[GLR_GUARD_CONSECUTIVE] = 0;
      rec[GLR_GUARD_SKIP] = 0;
    } else {
      long long f = rf[0] < rf[1] ? rf[0] : rf[1];
      f = rf[2] < f ? rf[2] : f;
      f = rf[3] < f ? rf[3] : f;
      const long long run = rec[GLR_GUARD_CONSECUTIVE] + 1;
      rec[GLR_GUARD_SKIPPED] += 1;
      rec[GLR_GUARD_CONSECUTIVE] = run;
      rec[GLR_GUARD_SKIP] = 1;
      rec[GLR_GUARD_LAST_CALL] = call;
      rec[GLR_GUARD_LAST_COUNT] = bad;
      rec[GLR_GUARD_LAST_PARTIAL] = f;
      rec[GLR_GUARD_LAST_OFFSET] = nf[2 * (size_t)f + 1];
      if (run > rec[GLR_GUARD_LONGEST]) rec[GLR_GUARD_LONGEST] = run;
    }
  }
}

// GUARD: nothing is written when the guard skipped this step; the bias corrections come from the host-built table at
// the applied-step count the guard has just advanced (bias[2 (t - 1)] = 1 - b1^t, bias[2 (t - 1) + 1] = sqrt(1 - b2^t)),
// i.e. the very floats the unguarded launch wrappers pass as bc1 / bc2_sqrt
__device__ __forceinline__ bool guard_skip(const long long* __restrict__ rec, const float* __restrict__ bias, int bias_cap,
                                           float& bc1, float& bc2_sqrt) {
  if (rec[GLR_GUARD_SKIP] != 0) return true;
  long long t = rec[GLR_GUARD_APPLIED];
  t = t < 1 ? 1 : (t > bias_cap ? bias_cap : t);
  bc1 = bias[2 * (t - 1)];
  bc2_sqrt = bias[2 * (t - 1) + 1];
  return false;
}

template <bool GUARD>
__global__ void __launch_bounds__(OPT_NT) k_adam(float* __restrict__ master, float* __restrict__ m, float* __restrict__ v,
                                                 const void* __restrict__ grad, int grad_dtype,
                                                 unsigned short* __restrict__ shadow, size_t n, float lr, float b1, float b2,
                                                 float eps, float wd, float bc1, float bc2_sqrt,
                                                 const float* __restrict__ clip, const long long* __restrict__ rec,
                                                 const float* __restrict__ bias, int bias_cap) {
  const size_t i = ((size_t)blockIdx.x * OPT_NT + threadIdx.x) * OPT_VEC;
  if (i >= n) return;
  if constexpr (GUARD) {
    if (guard_skip(rec, bias, bias_cap, bc1, bc2_sqrt)) return;
  }
  const float c = clip ? clip[1] : 1.f;
  float g[8], p[8], a[8], b[8];
  load8(grad, grad_dtype, i, g);
  load8(master, GLR_F32, i, p);
  load8(m, GLR_F32, i, a);
  load8(v, GLR_F32, i, b);
  const float step = lr / bc1;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float gk = __builtin_fmaf(wd, p[k], g[k] * c);             // torch.optim.Adam: grad + weight_decay * param
    a[k] = __builtin_fmaf(b1, a[k], (1.f - b1) * gk);
    b[k] = __builtin_fmaf(b2, b[k], (1.f - b2) * gk * gk);
    const float denom = sqrtf(b[k]) / bc2_sqrt + eps;
    p[k] = p[k] - step * (a[k] / denom);
  }
  *reinterpret_cast<float4*>(master + i) = make_float4(p[0], p[1], p[2], p[3]);
  *reinterpret_cast<float4*>(master + i + 4) = make_float4(p[4], p[5], p[6], p[7]);
  *reinterpret_cast<float4*>(m + i) = make_float4(a[0], a[1], a[2], a[3]);
  *reinterpret_cast<float4*>(m + i + 4) = make_float4(a[4], a[5], a[6], a[7]);
  *reinterpret_cast<float4*>(v + i) = make_float4(b[0], b[1], b[2], b[3]);
  *reinterpret_cast<float4*>(v + i + 4) = make_float4(b[4], b[5], b[6], b[7]);
  if (shadow) {
    uint4 u;
    u.x = f2bf(p[0]) | ((unsigned)f2bf(p[1]) << 16);
    u.y = f2bf(p[2]) | ((unsigned)f2bf(p[3]) << 16);
    u.z = f2bf(p[4]) | ((unsigned)f2bf(p[5]) << 16);
    u.w = f2bf(p[6]) | ((unsigned)f2bf(p[7]) << 16);
    *reinterpret_cast<uint4*>(shadow + i) = u;
  }
}

// ---- pointer-table forms: gradients stay where autograd left them (one tensor per parameter, no accumulation
// into a flat buffer: that costs an add launch per parameter).  One workgroup per chunk of <= OPT_CHUNK elements.
//   chunk[c] = { parameter index, element offset inside the parameter, element offset in the flat buffers, count }
//   gptr[param] = device address of the parameter's gradient this step (0: no gradient -> the parameter is skipped,
//   like torch.optim.Adam skips a None gradient)
struct ChunkEnt { int param; int count; long long poff; long long foff; };

__device__ __forceinline__ float ld1(const void* p, int dtype, size_t i) {
  return dtype == GLR_BF16 ? bf2f(reinterpret_cast<const unsigned short*>(p)[i]) : reinterpret_cast<const float*>(p)[i];
}

// GUARD: non-finite offsets are element offsets inside the chunk (0 .. count - 1)
template <bool GUARD>
__global__ void __launch_bounds__(OPT_NT) k_sumsq_mt(const ChunkEnt* __restrict__ chunk, const unsigned long long* __restrict__ gptr,
                                                     int dtype, float* __restrict__ partial, long long* __restrict__ nf) {
  __shared__ float red[OPT_NT / 64];
  const ChunkEnt e = chunk[blockIdx.x];
  const void* g = reinterpret_cast<const void*>(gptr[e.param]);
  float s = 0.f;
  BadSeen bad;
  if (g != nullptr) {
    const int nv = e.count & ~7;
    for (int i = threadIdx.x * OPT_VEC; i < nv; i += OPT_NT * OPT_VEC) {
      float v[8];
      load8(g, dtype, (size_t)e.poff + i, v);
#pragma unroll
      for (int k = 0; k < 8; ++k) s = __builtin_fmaf(v[k], v[k], s);
      if constexpr (GUARD) {
#pragma unroll
        for (int k = 0; k < 8; ++k) bad.see(v[k], i + k);
      }
    }
    for (int i = nv + threadIdx.x; i < e.count; i += OPT_NT) {
      const float x = ld1(g, dtype, (size_t)e.poff + i);
      s = __builtin_fmaf(x, x, s);
      if constexpr (GUARD) bad.see(x, i);
    }
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  if constexpr (GUARD) write_bad(bad, nf);
}

template <bool GUARD>
__global__ void __launch_bounds__(OPT_NT) k_adam_mt(const ChunkEnt* __restrict__ chunk, const unsigned long long* __restrict__ gptr,
                                                    int grad_dtype, float* __restrict__ master, float* __restrict__ m,
                                                    float* __restrict__ v, unsigned short* __restrict__ shadow, float lr,
                                                    float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt,
                                                    const float* __restrict__ clip, const long long* __restrict__ rec,
                                                    const float* __restrict__ bias, int bias_cap) {
  const ChunkEnt e = chunk[blockIdx.x];
  const void* gp = reinterpret_cast<const void*>(gptr[e.param]);
  if (gp == nullptr) return;
  if constexpr (GUARD) {
    if (guard_skip(rec, bias, bias_cap, bc1, bc2_sqrt)) return;
  }
  const float c = clip ? clip[1] : 1.f;
  const float step = lr / bc1;
  // chunks start 8-aligned in the flat buffers (parameters are padded to 8) and 8-aligned inside the parameter
  for (int i = threadIdx.x * OPT_VEC; i < e.count; i += OPT_NT * OPT_VEC) {
    const size_t f = (size_t)e.foff + i;
    float g[8], p[8], a[8], b[8];
    if (i + 8 <= e.count) {
      load8(gp, grad_dtype, (size_t)e.poff + i, g);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) g[k] = i + k < e.count ? ld1(gp, grad_dtype, (size_t)e.poff + i + k) : 0.f;
    }
    load8(master, GLR_F32, f, p);
    load8(m, GLR_F32, f, a);
    load8(v, GLR_F32, f, b);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float gk = __builtin_fmaf(wd, p[k], g[k] * c);
      a[k] = __builtin_fmaf(b1, a[k], (1.f - b1) * gk);
      b[k] = __builtin_fmaf(b2, b[k], (1.f - b2) * gk * gk);
      p[k] = p[k] - step * (a[k] / (sqrtf(b[k]) / bc2_sqrt + eps));
    }
    *reinterpret_cast<float4*>(master + f) = make_float4(p[0], p[1], p[2], p[3]);
    *reinterpret_cast<float4*>(master + f + 4) = make_float4(p[4], p[5], p[6], p[7]);
    *reinterpret_cast<float4*>(m + f) = make_float4(a[0], a[1], a[2], a[3]);
    *reinterpret_cast<float4*>(m + f + 4) = make_float4(a[4], a[5], a[6], a[7]);
    *reinterpret_cast<float4*>(v + f) = make_float4(b[0], b[1], b[2], b[3]);
    *reinterpret_cast<float4*>(v + f + 4) = make_float4(b[4], b[5], b[6], b[7]);
    if (shadow) {
      uint4 u;
      u.x = f2bf(p[0]) | ((unsigned)f2bf(p[1]) << 16);
      u.y = f2bf(p[2]) | ((unsigned)f2bf(p[3]) << 16);
      u.z = f2bf(p[4]) | ((unsigned)f2bf(p[5]) << 16);
      u.w = f2bf(p[6]) | ((unsigned)f2bf(p[7]) << 16);
      *reinterpret_cast<uint4*>(shadow + f) = u;
    }
  }
}

// gather: the gradients of a bucket's parameters (one tensor each) -> their slots of the flat gradient buffer, one
// launch per bucket (data-parallel: the bucket is then all-reduced as one slice)
__global__ void __launch_bounds__(OPT_NT) k_gather_mt(const ChunkEnt* __restrict__ chunk, const unsigned long long* __restrict__ gptr,
                                                      int dtype, void* __restrict__ flat) {
  const ChunkEnt e = chunk[blockIdx.x];
  const void* g = reinterpret_cast<const void*>(gptr[e.param]);
  if (g == nullptr) return;                        // the slot keeps the zeros of zero_grad
  const int esz = dtype == GLR_BF16 ? 2 : 4, per16 = 16 / esz;
  const unsigned char* src = reinterpret_cast<const unsigned char*>(g) + (size_t)e.poff * esz;
  unsigned char* dst = reinterpret_cast<unsigned char*>(flat) + (size_t)e.foff * esz;
  const int nv = e.count / per16;
  for (int i = threadIdx.x; i < nv; i += OPT_NT)
    reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
  for (int i = nv * per16 + threadIdx.x; i < e.count; i += OPT_NT) {
    if (esz == 2) reinterpret_cast<unsigned short*>(dst)[i] = reinterpret_cast<const unsigned short*>(src)[i];
    else reinterpret_cast<float*>(dst)[i] = reinterpret_cast<const float*>(src)[i];
  }
}

// accumulate: acc[foff + i] = scale * g (FIRST: the slot's old content is never read, a parameter without a gradient is
// written with zeros) or fmaf(scale, g, acc[foff + i]) (a parameter without a gradient keeps its slot) - one rounding
// per element either way, g the bf16 / fp32 gradient widened to fp32.  Only [foff, foff + count) is written: the padding
// between parameters keeps its zeros.  HBM-bound: 2 (4) + 4 bytes read, 4 written per element; FIRST saves the 4.
template <bool FIRST>
__global__ void __launch_bounds__(OPT_NT) k_accum_mt(const ChunkEnt* __restrict__ chunk, const unsigned long long* __restrict__ gptr,
                                                     int dtype, float* __restrict__ acc, float scale) {
  const ChunkEnt e = chunk[blockIdx.x];
  const void* g = reinterpret_cast<const void*>(gptr[e.param]);
  if (g == nullptr && !FIRST) return;
  float* dst = acc + e.foff;
  const int nv = e.count & ~7;
  // chunks start 8-aligned in the accumulator and inside the parameter: 16-byte accesses up to nv, scalars after it
  for (int i = threadIdx.x * OPT_VEC; i < nv; i += OPT_NT * OPT_VEC) {
    float v[8];
    if (g != nullptr) {
      load8(g, dtype, (size_t)e.poff + i, v);
      if constexpr (FIRST) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = scale * v[k];
      } else {
        float a[8];
        load8(dst, GLR_F32, (size_t)i, a);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = __builtin_fmaf(scale, v[k], a[k]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = 0.f;
    }
    *reinterpret_cast<float4*>(dst + i) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(dst + i + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
  for (int i = nv + threadIdx.x; i < e.count; i += OPT_NT) {
    float x = 0.f;
    if (g != nullptr) {
      x = ld1(g, dtype, (size_t)e.poff + i);
      x = FIRST ? scale * x : __builtin_fmaf(scale, x, dst[i]);
    }
    dst[i] = x;
  }
}

}  // namespace

extern "C" int glr_accum_mt(const void* chunk_table, int n_chunks, const uint64_t* grad_ptrs, int src_dtype, float* acc,
                            float scale, int first, void* stream) {
  if (!chunk_table || !grad_ptrs || !acc || n_chunks <= 0 || !std::isfinite(scale)) return GLR_EINVAL;
  if (src_dtype != GLR_F32 && src_dtype != GLR_BF16) return GLR_EDTYPE;
  if (first)
    hipLaunchKernelGGL(k_accum_mt<true>, dim3(n_chunks), dim3(OPT_NT), 0, (hipStream_t)stream, (const ChunkEnt*)chunk_table,
                       (const unsigned long long*)grad_ptrs, src_dtype, acc, scale);
  else
    hipLaunchKernelGGL(k_accum_mt<false>, dim3(n_chunks), dim3(OPT_NT), 0, (hipStream_t)stream, (const ChunkEnt*)chunk_table,
                       (const unsigned long long*)grad_ptrs, src_dtype, acc, scale);
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}

extern "C" int glr_gather_mt(const void* chunk_table, int n_chunks, const uint64_t* grad_ptrs, int dtype, void* flat,
                             void* stream) {
  if (!chunk_table || !grad_ptrs || !flat || n_chunks <= 0) return GLR_EINVAL;
  if (dtype != GLR_F32 && dtype != GLR_BF16) return GLR_EDTYPE;
  hipLaunchKernelGGL(k_gather_mt, dim3(n_chunks), dim3(OPT_NT), 0, (hipStream_t)stream, (const ChunkEnt*)chunk_table,
                     (const unsigned long long*)grad_ptrs, dtype, flat);
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}

extern "C" int glr_sumsq_mt(const void* chunk_table, int n_chunks, const uint64_t* grad_ptrs, int dtype, float* partial,
                            void* stream) {
  if (!chunk_table || !grad_ptrs || !partial || n_chunks <= 0) return GLR_EINVAL;
  if (dtype != GLR_F32 && dtype != GLR_BF16) return GLR_EDTYPE;
  hipLaunchKernelGGL(k_sumsq_mt<false>, dim3(n_chunks), dim3(OPT_NT), 0, (hipStream_t)stream, (const ChunkEnt*)chunk_table,
                     (const unsigned long long*)grad_ptrs, dtype, partial, nullptr);
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}

extern "C" int glr_sumsq_mt_g(const void* chunk_table, int n_chunks, const uint64_t* grad_ptrs, int dtype, float* partial,
                              int64_t* nonfinite, void* stream) {
  if (!chunk_table || !grad_ptrs || !partial || !nonfinite || n_chunks <= 0) return GLR_EINVAL;
  if (dtype != GLR_F32 && dtype != GLR_BF16) return GLR_EDTYPE;
  hipLaunchKernelGGL(k_sumsq_mt<true>, dim3(n_chunks), dim3(OPT_NT), 0, (hipStream_t)stream, (const ChunkEnt*)chunk_table,
                     (const unsigned long long*)grad_ptrs, dtype, partial, (long long*)nonfinite);
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}

extern "C" int glr_adam_step_mt(const void* chunk_table, int n_chunks, const uint64_t* grad_ptrs, int grad_dtype,
                                float* master, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, float lr, float beta1,
                                float beta2, float eps, float weight_decay, int step, const float* clip, void* stream) {
  if (!chunk_table || !grad_ptrs || !master || !exp_avg || !exp_avg_sq || n_chunks <= 0 || step < 1) return GLR_EINVAL;
  if (grad_dtype != GLR_F32 && grad_dtype != GLR_BF16) return GLR_EDTYPE;
  const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  hipLaunchKernelGGL(k_adam_mt<false>, dim3(n_chunks), dim3(OPT_NT), 0, (hipStream_t)stream, (const ChunkEnt*)chunk_table,
                     (const unsigned long long*)grad_ptrs, grad_dtype, master, exp_avg, exp_avg_sq,
                     (unsigned short*)shadow_bf16, lr, beta1, beta2, eps, weight_decay, bc1, sqrtf(bc2), clip, nullptr,
                     nullptr, 0);
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}

extern "C" int glr_adam_step_mt_g(const void* chunk_table, int n_chunks, const uint64_t* grad_ptrs, int grad_dtype,
                                  float* master, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, float lr, float beta1,
                                  float beta2, float eps, float weight_decay, const float* bias_table, int bias_capacity,
                                  const int64_t* record, const float* clip, void* stream) {
  if (!chunk_table || !grad_ptrs || !master || !exp_avg || !exp_avg_sq || !bias_table || !record || n_chunks <= 0 ||
      bias_capacity < 1)
    return GLR_EINVAL;
  if (grad_dtype != GLR_F32 && grad_dtype != GLR_BF16) return GLR_EDTYPE;
  hipLaunchKernelGGL(k_adam_mt<true>, dim3(n_chunks), dim3(OPT_NT), 0, (hipStream_t)stream, (const ChunkEnt*)chunk_table,
                     (const unsigned long long*)grad_ptrs, grad_dtype, master, exp_avg, exp_avg_sq,
                     (unsigned short*)shadow_bf16, lr, beta1, beta2, eps, weight_decay, 1.f, 1.f, clip,
                     (const long long*)record, bias_table, bias_capacity);
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}

extern "C" int glr_sumsq_blocks(long long n) {
  if (n <= 0) return GLR_EINVAL;
  const long long b = (n / OPT_VEC + OPT_NT * 8 - 1) / (OPT_NT * 8);       // >= 8 trips per thread
  return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

extern "C" int glr_sumsq_partial(const void* x, int dtype, long long n, float* partial, void* stream) {
  if (!x || !partial || n <= 0 || n % OPT_VEC != 0) return GLR_EINVAL;
  if (dtype != GLR_F32 && dtype != GLR_BF16) return GLR_EDTYPE;
  hipLaunchKernelGGL(k_sumsq<false>, dim3(glr_sumsq_blocks(n)), dim3(OPT_NT), 0, (hipStream_t)stream, x, dtype, (size_t)n,
                     partial, nullptr);
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}

extern "C" int glr_sumsq_partial_g(const void* x, int dtype, long long n, float* partial, int64_t* nonfinite, void* stream) {
  if (!x || !partial || !nonfinite || n <= 0 || n % OPT_VEC != 0) return GLR_EINVAL;
  if (dtype != GLR_F32 && dtype != GLR_BF16) return GLR_EDTYPE;
  hipLaunchKernelGGL(k_sumsq<true>, dim3(glr_sumsq_blocks(n)), dim3(OPT_NT), 0, (hipStream_t)stream, x, dtype, (size_t)n,
                     partial, (long long*)nonfinite);
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}

extern "C" int glr_clip_coef(const float* partial, int n_partial, float max_norm, float* out, void* stream) {
  if (!partial || !out || n_partial <= 0) return GLR_EINVAL;
  hipLaunchKernelGGL(k_clip_coef, dim3(1), dim3(OPT_NT), 0, (hipStream_t)stream, partial, n_partial, max_norm, out);
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}

extern "C" int glr_step_guard(const float* partial, const int64_t* nonfinite, int n_partial, float max_norm, float* out,
                              int64_t* record, long long call_index, void* stream) {
  if (!partial || !nonfinite || !out || !record || n_partial <= 0) return GLR_EINVAL;
  hipLaunchKernelGGL(k_step_guard, dim3(1), dim3(OPT_NT), 0, (hipStream_t)stream, partial, (const long long*)nonfinite,
                     n_partial, max_norm, out, (long long*)record, call_index);
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}

extern "C" int glr_adam_step(float* master, float* exp_avg, float* exp_avg_sq, const void* grad, int grad_dtype,
                             void* shadow_bf16, long long n, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int step, const float* clip, void* stream) {
  if (!master || !exp_avg || !exp_avg_sq || !grad || n <= 0 || n % OPT_VEC != 0 || step < 1) return GLR_EINVAL;
  if (grad_dtype != GLR_F32 && grad_dtype != GLR_BF16) return GLR_EDTYPE;
  const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  const size_t threads = (size_t)n / OPT_VEC;
  hipLaunchKernelGGL(k_adam<false>, dim3((unsigned)((threads + OPT_NT - 1) / OPT_NT)), dim3(OPT_NT), 0, (hipStream_t)stream,
                     master, exp_avg, exp_avg_sq, grad, grad_dtype, (unsigned short*)shadow_bf16, (size_t)n, lr, beta1,
                     beta2, eps, weight_decay, bc1, sqrtf(bc2), clip, nullptr, nullptr, 0);
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}

extern "C" int glr_adam_step_g(float* master, float* exp_avg, float* exp_avg_sq, const void* grad, int grad_dtype,
                               void* shadow_bf16, long long n, float lr, float beta1, float beta2, float eps,
                               float weight_decay, const float* bias_table, int bias_capacity, const int64_t* record,
                               const float* clip, void* stream) {
  if (!master || !exp_avg || !exp_avg_sq || !grad || !bias_table || !record || n <= 0 || n % OPT_VEC != 0 ||
      bias_capacity < 1)
    return GLR_EINVAL;
  if (grad_dtype != GLR_F32 && grad_dtype != GLR_BF16) return GLR_EDTYPE;
  const size_t threads = (size_t)n / OPT_VEC;
  hipLaunchKernelGGL(k_adam<true>, dim3((unsigned)((threads + OPT_NT - 1) / OPT_NT)), dim3(OPT_NT), 0, (hipStream_t)stream,
                     master, exp_avg, exp_avg_sq, grad, grad_dtype, (unsigned short*)shadow_bf16, (size_t)n, lr, beta1,
                     beta2, eps, weight_decay, 1.f, 1.f, clip, (const long long*)record, bias_table, bias_capacity);
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}

// host only: the bias corrections of steps 1 .. capacity by the expressions of the launch wrappers above, so that the
// guarded kernels use bitwise the floats the unguarded ones are handed
extern "C" int glr_adam_bias_table(float beta1, float beta2, int capacity, float* out) {
  if (!out || capacity < 1) return GLR_EINVAL;
  for (int step = 1; step <= capacity; ++step) {
    const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
    out[2 * (size_t)(step - 1)] = bc1;
    out[2 * (size_t)(step - 1) + 1] = sqrtf(bc2);
  }
  return GLR_OK;
}
