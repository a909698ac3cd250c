// Feed-forward middle of a post-LN transformer encoder layer,  a = dropout(relu(z)),  z = linear1(x) (bias included), for the
// image-region transformer (reference: the nn.TransformerEncoder of gloria/models/gloria_model.py:52-59 run under native
// AMP; its layers compute linear2(dropout(relu(linear1(x))))), forward and backward.
//
// Under autocast torch runs this as relu (read + write), dropout (read + write + a byte mask) and, backward, dropout backward,
// threshold backward and the bias-gradient reduction of linear1: ~9 and ~13 bytes per element of the [R, C] intermediate.
// Fused, one pass per direction:
//   forward   read z (bf16); write a (bf16) + 1 bit `alive = kept && z > 0`                           4 B + 1 bit
//   backward  read dy (bf16) + the bit; write dz (bf16); column sums of dz on the way (linear1's db)    4 B + 1 bit
// z is not kept for the backward: the bit is all it needs.  The bit layout is glr_drop_add_ln_fwd's (element 4 (l + 64 i) + c
// of a row = bit l of word 4 i + c), so lane l owns the 4 consecutive elements of quad l + 64 i: 8-byte loads and stores, mask
// words from wave ballots.  Dropout bits: Philox4x32-10, counter = row * (C / 4) + quad, as glr_lnorm.hip - a pure function
// of (key, row, column).  The forward with dropout is bound by Philox's 40 quarter-rate multiplies per quad, not by HBM.
// Column sums: per-lane registers over the workgroup's row slab -> LDS over its four waves -> partial [C][n_part] -> a
// fixed-order second stage.  No atomics: bitwise reproducible.
#include "glr_common.h"

namespace {

constexpr int FF_NT = 256;             // four waves
constexpr int FF_MAX_C = 4096;         // 64 mask words per row: one per lane

// one wave per row, NQ = C / 256 quads per lane, four 8-byte loads in flight
template <bool DROP>
__global__ void __launch_bounds__(FF_NT) k_relu_drop_fwd(const unsigned short* __restrict__ z, long long R, int nq, float p_drop,
                                                         float s, unsigned seed_lo, unsigned seed_hi, unsigned off_lo,
                                                         unsigned off_hi, const unsigned long long* __restrict__ rng,
                                                         unsigned short* __restrict__ a, unsigned long long* __restrict__ alive) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (FF_NT / 64) + (threadIdx.x >> 6);
  if (row >= R) return;
  unsigned thr = 0u;
  if (DROP) {
    if (rng != nullptr) {        // key from device memory (hipGraph replays), as glr_lnorm.hip
      const unsigned long long sd = rng[0], o = rng[1] + (((unsigned long long)off_hi << 32) | off_lo);
      seed_lo = (unsigned)sd; seed_hi = (unsigned)(sd >> 32); off_lo = (unsigned)o; off_hi = (unsigned)(o >> 32);
    }
    thr = (unsigned)fminf(p_drop * 4294967296.f, 4294967040.f);
  }
  const long long C = (long long)nq * 256;
  const uint2* __restrict__ zr = reinterpret_cast<const uint2*>(z + row * C);
  uint2* __restrict__ ar = reinterpret_cast<uint2*>(a + row * C);
  unsigned long long myword = 0ull;
  for (int i0 = 0; i0 < nq; i0 += 4) {
    uint2 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i0 + u < nq) v[u] = zr[lane + 64 * (i0 + u)];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u;
      if (i >= nq) break;                      // wave-uniform
      const int quad = lane + 64 * i;
      float zv[4], av[4];
      unpack4(v[u], zv);
      unsigned rr[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
      if (DROP) {
        const unsigned long long ctr = (unsigned long long)row * (unsigned long long)(C / 4) + quad;
        const U4 rnd = philox4x32((unsigned)ctr, (unsigned)(ctr >> 32), off_lo, off_hi, seed_lo, seed_hi);
        rr[0] = rnd.x; rr[1] = rnd.y; rr[2] = rnd.z; rr[3] = rnd.w;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool live = rr[c] >= thr && zv[c] > 0.f;
        av[c] = live ? zv[c] * s : 0.f;
        if (alive != nullptr) {
          const unsigned long long word = __ballot(live);
          if (lane == i * 4 + c) myword = word;
        }
      }
      ar[quad] = pack4(av);
    }
  }
  if (alive != nullptr && lane < nq * 4) alive[row * (nq * 4) + lane] = myword;
}

// workgroup = one 256-column block x one row slab; wave w takes rows r0 + w, r0 + w + 4, ..., four rows in flight
__global__ void __launch_bounds__(FF_NT) k_relu_drop_bwd(const unsigned short* __restrict__ dy, const unsigned long long* __restrict__ alive,
                                                         long long R, int nq, float s, long long rows_per,
                                                         unsigned short* __restrict__ dz, float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // rows are wave-uniform: mask words by scalar loads
  const int i = blockIdx.x;
  const long long C = (long long)nq * 256;
  const long long r0 = (long long)blockIdx.y * rows_per;
  const long long r1 = r0 + rows_per < R ? r0 + rows_per : R;
  const long long col = 4 * (lane + 64 * i);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (long long rb = r0 + wv; rb < r1; rb += 16) {
    uint2 v[4];
    unsigned long long w[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long r = rb + 4 * u;
      if (r < r1) {                            // wave-uniform
        v[u] = *reinterpret_cast<const uint2*>(dy + r * C + col);
        const unsigned long long* mw = alive + r * (nq * 4) + 4 * i;
#pragma unroll
        for (int c = 0; c < 4; ++c) w[u][c] = mw[c];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long r = rb + 4 * u;
      if (r >= r1) break;
      float dv[4], o[4];
      unpack4(v[u], dv);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        o[c] = ((w[u][c] >> lane) & 1ull) ? dv[c] * s : 0.f;
        acc[c] += bf2f(f2bf(o[c]));            // the sum of what is stored
      }
      *reinterpret_cast<uint2*>(dz + r * C + col) = pack4(o);
    }
  }
  if (part == nullptr) return;
  __shared__ float red[FF_NT / 64][256];
#pragma unroll
  for (int c = 0; c < 4; ++c) red[wv][4 * lane + c] = acc[c];
  __syncthreads();
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < FF_NT / 64; ++k) sum += red[k][threadIdx.x];
  part[((size_t)i * 256 + threadIdx.x) * gridDim.y + blockIdx.y] = sum;
}

// second stage: one wave per column sums its partials in a fixed order
__global__ void __launch_bounds__(FF_NT) k_ffn_finish(const float* __restrict__ part, int n_part, int C, void* __restrict__ out,
                                                      int out_bf16) {
  const int lane = threadIdx.x & 63;
  const int col = blockIdx.x * (FF_NT / 64) + (threadIdx.x >> 6);
  if (col >= C) return;
  float e = 0.f;
  for (int k = lane; k < n_part; k += 64) e += part[(size_t)col * n_part + k];
  e = wave_sum(e);
  if (lane == 0) {
    if (out_bf16) reinterpret_cast<unsigned short*>(out)[col] = f2bf(e);
    else reinterpret_cast<float*>(out)[col] = e;
  }
}

bool ffn_shape_ok(long long R, int C) {
  return R >= 1 && R <= 4ll * 0x7fffffff && C >= 256 && C <= FF_MAX_C && C % 256 == 0;
}
int ffn_parts(long long R, int C) {                    // row slabs: ~8 workgroups per CU over the grid, >= 16 rows each
  const long long np = 2048 / (C / 256);
  const long long max_np = (R + 15) / 16;
  return (int)(np < max_np ? np : max_np);
}

}  // namespace

extern "C" int glr_ffn_workspace_floats(long long R, int C) { return ffn_shape_ok(R, C) ? ffn_parts(R, C) * C : 0; }

extern "C" int glr_relu_drop_fwd(const void* z16, long long R, int C, float p_drop, unsigned long long seed,
                                 unsigned long long offset, const unsigned long long* rng_cell, void* a16,
                                 unsigned long long* alive, void* stream) {
  if (!z16 || !a16 || !ffn_shape_ok(R, C)) return GLR_EINVAL;
  if (!(p_drop >= 0.f) || p_drop >= 1.f || (p_drop > 0.f && !alive)) return GLR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const float s = 1.0f / (1.0f - p_drop);
  const int grid = (int)((R + FF_NT / 64 - 1) / (FF_NT / 64));
#define GLR_FF_FWD(DROP)                                                                                                      \
  hipLaunchKernelGGL((k_relu_drop_fwd<DROP>), dim3(grid), dim3(FF_NT), 0, st, (const unsigned short*)z16, R, C / 256, p_drop, s, \
                     (unsigned)seed, (unsigned)(seed >> 32), (unsigned)offset, (unsigned)(offset >> 32), rng_cell,           \
                     (unsigned short*)a16, alive)
  if (p_drop > 0.f) GLR_FF_FWD(true);
  else GLR_FF_FWD(false);
#undef GLR_FF_FWD
  GLR_CHECK_LAUNCH();
  return GLR_OK;
}

extern "C" int glr_relu_drop_bwd(const void* dy16, const unsigned long long* alive, long long R, int C, float p_drop, void* dz16,
                                 float* workspace, void* dzsum, int dzsum_bf16, void* stream) {
  if (!dy16 || !alive || !dz16 || !ffn_shape_ok(R, C) || (dzsum && !workspace)) return GLR_EINVAL;
  if (!(p_drop >= 0.f) || p_drop >= 1.f) return GLR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const float s = 1.0f / (1.0f - p_drop);
  const int np = ffn_parts(R, C);
  const long long rows_per = (R + np - 1) / np;
  hipLaunchKernelGGL(k_relu_drop_bwd, dim3(C / 256, np), dim3(FF_NT), 0, st, (const unsigned short*)dy16, alive, R, C / 256, s,
                     rows_per, (unsigned short*)dz16, dzsum ? workspace : nullptr);
  GLR_CHECK_LAUNCH();
  if (dzsum) {
    hipLaunchKernelGGL(k_ffn_finish, dim3((C + FF_NT / 64 - 1) / (FF_NT / 64)), dim3(FF_NT), 0, st, workspace, np, C, dzsum, dzsum_bf16);
    GLR_CHECK_LAUNCH();
  }
  return GLR_OK;
}
