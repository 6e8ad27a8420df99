// mke_attr_conv.h — the phases of the attribute CNN's convolution kernels (mke_attr_cnn.hip composes them into four kernels).
//
// One group of LPT lanes per triple, lane = width position (WPL positions per lane: w = tl + LPT * i), rows staged through
// per-group LDS strips for the +-2 neighbour reads.  The backward recomputes the (cheap) forward instead of storing
// activations (conv_forward_triple is shared by both directions), back-propagates through both convolutions, the width
// normalisation and the batch-norm affine, scatters the attribute-row gradient with atomics and block-reduces the parameter
// gradients.  Every function here is inlined into its kernel; the kernels own the LDS and hand out pointers.
#pragma once
#include <type_traits>
#include "mke_gemm.h"

namespace mke {

#define CNN_BN_EPS 1e-3f
#define CNN_NCONV 52  // K1 16 + b1 2 + K2 32 + b2 2
#define CNN_WS_COPIES 32
#define CNN_WS_STRIDE(d) (2 * (d) + 64)  // MKE_CNN_WORKSPACE_FLOATS(dim) = copies * stride

typedef float v2f __attribute__((ext_vector_type(2)));

// The LDS strips of the convolution kernels are private to a wavefront: ordering its own LDS writes before its own later reads
// needs no block barrier, only that the writes have been issued to the LDS (in-order per wave) and that the compiler does not
// move the reads up.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// every block adds up the MKE_LOSS_PARTIALS partials of the previous kernel itself: NA arrays at once (one pass over all of
// them, one pair of barriers)
template <int NA>
__device__ __forceinline__ void totals_of_partials(const double* const (&parts)[NA], double (&tot)[NA]) {
  __shared__ double s_t[NA];
  __shared__ double s_w[NA][MKE_BLOCK / 64];
  double v[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) v[a] = 0.0;
  for (int i = threadIdx.x; i < MKE_LOSS_PARTIALS; i += MKE_BLOCK) {
#pragma unroll
    for (int a = 0; a < NA; ++a) v[a] += parts[a][i];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int a = 0; a < NA; ++a) v[a] += __shfl_down(v[a], off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < NA; ++a) s_w[a][threadIdx.x >> 6] = v[a];
  }
  __syncthreads();
  if (threadIdx.x < NA) {
    double t = 0.0;
    for (int w = 0; w < MKE_BLOCK / 64; ++w) t += s_w[threadIdx.x][w];
    s_t[threadIdx.x] = t;
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < NA; ++a) tot[a] = s_t[a];
}

__device__ __forceinline__ double total_of_partials(const double* __restrict__ partials) {
  const double* const parts[1] = {partials};
  double tot[1];
  totals_of_partials<1>(parts, tot);
  return tot[0];
}

// the two batch-wide scalars of dz_of from the per-block partials: S = sum z^2, T = sum g . z over the whole batch
__device__ __forceinline__ void batch_scalars(const double* __restrict__ ssq, const double* __restrict__ dotp, float& inv, float& coef) {
  const double* const parts[2] = {ssq, dotp};
  double tot[2];
  totals_of_partials<2>(parts, tot);
  const float S = (float)tot[0], T = (float)tot[1];
  inv = rsqrtf(fmaxf(S, MKE_L2_EPS));
  coef = S > MKE_L2_EPS ? T * inv * inv : 0.f;  // out * (g.out) = z * inv^2 * T
}

struct ConvParams {
  const float* __restrict__ attr;
  int attr_stride, attr_norm;
  const float* __restrict__ lit;
  int lit_stride;
  int dim;
  const int32_t* __restrict__ ia;
  const int32_t* __restrict__ iv;
  int64_t n;
  const float* __restrict__ params;  // packed: gamma[d] beta[d] K1[16] b1[2] K2[32] b2[2] ...
  float* __restrict__ flat;          // fwd out [n][flat_stride]; column 4d = 1 when flat_stride > 4d
  int flat_stride;
  const float* __restrict__ dflat;   // bwd in  [n][4d]
  float* __restrict__ gparams;       // bwd out, same packing, atomically accumulated
  float* __restrict__ gattr;         // bwd out: attribute-table gradient scratch (nullable)
  int gattr_copies;                  // >= 1: the scratch is [copies][n_attr][attr_stride], triple t adds to copy t % copies (a few hundred
  int64_t gattr_copy_elems;          // attribute rows take 5,000 triples per step and their frequencies are heavy-tailed)
  int32_t* __restrict__ tattr;
  int32_t tag;
  float* __restrict__ ws;            // bwd: MKE_CNN_WORKSPACE_FLOATS(dim) zero-invariant floats (nullable)
};

// fwd with the dense layer in the same launch (k_attr_conv_fwd_dense): z = tanh([flat, 1] W), W [4 dim + 1][dim]
struct DenseExtra {
  const float* __restrict__ W;
  float* __restrict__ z;
  double* __restrict__ ssq;          // per-block sums of z^2 (MKE_LOSS_PARTIALS slots; the ones no block owns are cleared)
};

// bwd with the dflat product in the block (k_attr_conv_bwd_fused): dflat tile = 16 rows of dz x W^T; the blocks behind the first
// conv_blocks of the grid are riders that compute the weight-gradient product `tall` ([flat, 1]^T dz over K splits)
struct FusedExtra {
  const float* __restrict__ dz;      // [n][dim]: g = dL/dout-side gradient of the loss tail (dz = dz_of(g, z, S, T) is formed on load)
  const float* __restrict__ zmat;    // [n][dim] z
  const double* __restrict__ ssq;    // per-block sums of z^2 and of g . z: the two batch-wide scalars of the transform
  const double* __restrict__ dotp;
  const float* __restrict__ wt;      // W^T [dim][4 dim]: the transposed copy k_attr_tail_loss left
  int conv_blocks;
  GemmParams tall;
};

// K1[kh][kw][0][f] at k1[(kh*4+kw)*2+f]; K2[kh][kw][c][f] at k2[((kh*4+kw)*2+c)*2+f]  (TF HWIO order)
// LPT lanes per triple (64: a wavefront per triple; 32: one per HALF — dim 75 fills 75 of 128 lane slots in two passes of 64
// lanes but 75 of 96 in three passes of 32, and a wavefront then carries two triples: a quarter fewer instructions per
// triple; 16: a quarter-wave per triple, 16 triples per block = the rows of one 16 x 16 MFMA tile), WPL width positions per
// lane: position w = tl + LPT * i of lane tl of the group.
// NW wavefronts per block (4; the two-triples-per-wavefront backward: 2 — each convolution kernel costs the latency chain of
// one block plus ~2 us per further 4-wavefront block on the same CU (batch-size scan in profiles/r02_attr_step.md); 5000
// triples are 625 such blocks = three on 113 of the 256 CUs, but 1250 half blocks = at most five halves per CU)
template <int WPL_, int LPT_, int NW_>
struct ConvShape {
  static constexpr int WPL = WPL_, LPT = LPT_, NW = NW_;
  static constexpr int NT = NW * 64;                      // threads per block
  static constexpr int TPW = 64 / LPT;                    // triples per wavefront
  static constexpr int NSLOT = NW * TPW;                  // triples in flight per block, each with its own LDS strips
  static constexpr int DP = LPT * WPL + 4;
  // LPT = 16: a half-wave reads two triples' strips at once — their distance must be 16 banks (mod 32) for the two 16-lane
  // runs not to overlap: 4 DP already is (the c1 strips); the x strips get their own row length (2 DPX = 16 mod 32)
  static constexpr int DPX = LPT == 16 ? DP + ((8 - DP % 16) + 16) % 16 : DP;
  int lane, wv;
  int tl;     // lane inside the triple's group
  int slot;   // which of the block's triples
  __device__ __forceinline__ ConvShape() : lane(threadIdx.x & 63), wv(threadIdx.x >> 6) {
    tl = lane & (LPT - 1);
    slot = wv * TPW + lane / LPT;
  }
  __device__ __forceinline__ int64_t first_triple() const { return (int64_t)blockIdx.x * NSLOT + slot; }
  static __device__ __forceinline__ float group_sum(float v) {   // over the LPT lanes of a triple
    v = sub16_sum(v);
    if (LPT >= 32) v += __shfl_xor(v, 16, 64);
    if (LPT == 64) v += __shfl_xor(v, 32, 64);
    return v;
  }
  // zero pads of a strip row whose index FRONT <-> width 0: FRONT in front, 4 - FRONT behind the LPT * WPL positions
  template <int FRONT>
  __device__ __forceinline__ void zero_halo(float* row) const {
    if (tl < 4) row[tl < FRONT ? tl : LPT * WPL + tl] = 0.f;
  }
};

template <int WPL>
struct ConvWeights {
  float k1[16], b1[2], k2[32], b2[2], gam[WPL], bet[WPL];
  template <int LPT>
  __device__ __forceinline__ void load(const float* __restrict__ params, int d, int tl) {
    const float* __restrict__ gamma = params;
    const float* __restrict__ beta = params + d;
    const float* cp = params + 2 * d;
#pragma unroll
    for (int i = 0; i < 16; ++i) k1[i] = cp[i];
    b1[0] = cp[16]; b1[1] = cp[17];
#pragma unroll
    for (int i = 0; i < 32; ++i) k2[i] = cp[18 + i];
    b2[0] = cp[50]; b2[1] = cp[51];
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      const int w = tl + LPT * i;
      gam[i] = w < d ? gamma[w] : 0.f;
      bet[i] = w < d ? beta[w] : 0.f;
    }
  }
};

// what the forward of one triple leaves in registers (the backward needs all of it)
template <int WPL>
struct ConvActs {
  float raw[2][WPL], c1[2][2][WPL], c2[2][2][WPL], nrm[2][2], ssq[2][2];
};

// gather (optionally l2-normalised attribute row, literal row) -> BN affine -> conv1 -> conv2 -> width normalisation factors.
// Leaves x in xs (index w+1 <-> width w) and c1 in c1s (likewise), both with zero pads.
template <class S>
__device__ __forceinline__ void conv_forward_triple(const ConvParams& p, const S& sh, const ConvWeights<S::WPL>& wt, int ra, int rv, bool live,
                                                    float (*xs)[S::DPX], float (*c1s)[2][S::DP], ConvActs<S::WPL>& a) {
  constexpr int WPL = S::WPL, LPT = S::LPT;
  const int d = p.dim, tl = sh.tl;
  const float bn_s = rsqrtf(1.0f + CNN_BN_EPS);
#pragma unroll
  for (int i = 0; i < WPL; ++i) {
    const int w = tl + LPT * i;
    a.raw[0][i] = (live && w < d) ? p.attr[(int64_t)ra * p.attr_stride + w] : 0.f;
    a.raw[1][i] = (live && w < d) ? p.lit[(int64_t)rv * p.lit_stride + w] : 0.f;
  }
  if (p.attr_norm) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < WPL; ++i) s = fmaf(a.raw[0][i], a.raw[0][i], s);
    s = S::group_sum(s);
    const float inv = rsqrtf(fmaxf(s, MKE_L2_EPS));
#pragma unroll
    for (int i = 0; i < WPL; ++i) a.raw[0][i] *= inv;
  }
  // ---- batch-norm affine, stage x with zero pads: index w+1 <-> width w ---------------------------------
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      const int w = tl + LPT * i;
      xs[h][w + 1] = w < d ? fmaf(wt.gam[i] * bn_s, a.raw[h][i], wt.bet[i]) : 0.f;
    }
    sh.template zero_halo<1>(xs[h]);
  }
  wave_lds_sync();
  // ---- conv1 ---------------------------------------------------------------------------------------------
#pragma unroll
  for (int i = 0; i < WPL; ++i) {
    const int w = tl + LPT * i;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // the two filters of a tap are adjacent in the packed weights: one v_pk_fma_f32 per tap for both (the input broadcast)
      v2f acc = {wt.b1[0], wt.b1[1]};
#pragma unroll
      for (int kh = 0; kh + h < 2; ++kh)
#pragma unroll
        for (int kw = 0; kw < 4; ++kw) {
          const float x = xs[h + kh][w + kw];
          acc = __builtin_elementwise_fma(v2f{wt.k1[(kh * 4 + kw) * 2], wt.k1[(kh * 4 + kw) * 2 + 1]}, v2f{x, x}, acc);
        }
      a.c1[h][0][i] = w < d ? tanh_f(acc.x) : 0.f;
      a.c1[h][1][i] = w < d ? tanh_f(acc.y) : 0.f;
      c1s[h][0][w + 1] = a.c1[h][0][i];
      c1s[h][1][w + 1] = a.c1[h][1][i];
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int f = 0; f < 2; ++f) sh.template zero_halo<1>(c1s[h][f]);
  wave_lds_sync();
  // ---- conv2 + width normalisation -----------------------------------------------------------------------
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int f = 0; f < 2; ++f) a.ssq[h][f] = 0.f;
#pragma unroll
  for (int i = 0; i < WPL; ++i) {
    const int w = tl + LPT * i;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      v2f acc = {wt.b2[0], wt.b2[1]};
#pragma unroll
      for (int kh = 0; kh + h < 2; ++kh)
#pragma unroll
        for (int kw = 0; kw < 4; ++kw)
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const float x = c1s[h + kh][c][w + kw];
            const int ki = ((kh * 4 + kw) * 2 + c) * 2;
            acc = __builtin_elementwise_fma(v2f{wt.k2[ki], wt.k2[ki + 1]}, v2f{x, x}, acc);
          }
      a.c2[h][0][i] = w < d ? tanh_f(acc.x) : 0.f;
      a.c2[h][1][i] = w < d ? tanh_f(acc.y) : 0.f;
      a.ssq[h][0] = fmaf(a.c2[h][0][i], a.c2[h][0][i], a.ssq[h][0]);
      a.ssq[h][1] = fmaf(a.c2[h][1][i], a.c2[h][1][i], a.ssq[h][1]);
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      a.ssq[h][f] = S::group_sum(a.ssq[h][f]);
      a.nrm[h][f] = rsqrtf(fmaxf(a.ssq[h][f], MKE_L2_EPS));
    }
}

// flat row of triple t (index h*2d + w*2 + c) to memory; TILE: also into the block's LDS tile row (dead rows as zeros), the A
// operand of the dense layer
template <bool TILE, class S>
__device__ __forceinline__ void conv_store_flat(const ConvParams& p, const S& sh, const ConvActs<S::WPL>& a, int64_t t, bool live,
                                                float* tile_row) {
  constexpr int WPL = S::WPL, LPT = S::LPT;
  const int d = p.dim, tl = sh.tl;
  if constexpr (TILE) {
    if (tl == 0) tile_row[4 * d] = live ? 1.0f : 0.f;
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      const int w = tl + LPT * i;
      if (w < d) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          tile_row[h * 2 * d + w * 2] = live ? a.c2[h][0][i] * a.nrm[h][0] : 0.f;
          tile_row[h * 2 * d + w * 2 + 1] = live ? a.c2[h][1][i] * a.nrm[h][1] : 0.f;
        }
      }
    }
  }
  if (live) {
    float* o = p.flat + t * (int64_t)p.flat_stride;
    if (tl == 0 && p.flat_stride > 4 * d) o[4 * d] = 1.0f;  // bias column: [flat, 1] @ [W; bias]
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      const int w = tl + LPT * i;
      if (w < d) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          float2 v = make_float2(a.c2[h][0][i] * a.nrm[h][0], a.c2[h][1][i] * a.nrm[h][1]);
          *reinterpret_cast<float2*>(o + h * 2 * d + w * 2) = v;
        }
      }
    }
  }
}

// Where the conv-parameter gradients wait for the block-level reduction (gamma / beta are per width position: registers of the kernel).
// The 52 conv-parameter gradients are NOT kept in registers: each is reduced over its quarter-wave as soon as it is
// formed and added to the quarter's own LDS slot (part).  48 + 4 long-lived accumulators pushed the backward kernel to
// 208 unified registers = 2 waves per SIMD = three rounds of waves for 5000 triples.
template <class S>
struct ParamGradSlots {
  typedef float Part[CNN_NCONV][4 * S::NW + 1];
  float (*part)[4 * S::NW + 1];
  int pq;
  bool plead;
  __device__ __forceinline__ ParamGradSlots(Part& s_part, const S& sh) : part(s_part), pq((sh.lane >> 4) + 4 * sh.wv), plead((sh.lane & 15) == 0) {
    for (int i = threadIdx.x; i < CNN_NCONV * (4 * S::NW + 1); i += S::NT) (&s_part[0][0])[i] = 0.f;
    __syncthreads();
  }
  __device__ __forceinline__ void park(int idx, float v) const {
    v = sub16_sum(v);
    if (plead) atomicAdd(&part[idx][pq], v);   // the slot belongs to this quarter-wave: no contention
  }
};

// one output position of a transposed 2x4 convolution with CIN input channels: sum over the taps of K[kh][kw][c][.] times the
// two filters' gradients ds[hh - kh][.][w + 3 - kw] (index w+2 <-> width w); the two filters' terms side by side, added at the end
template <int CIN, class S>
__device__ __forceinline__ float conv_transposed(const float* k, const float (*ds)[2][S::DP], int hh, int c, int w) {
  v2f acc2 = {0.f, 0.f};
#pragma unroll
  for (int kh = 0; kh <= hh; ++kh)
#pragma unroll
    for (int kw = 0; kw < 4; ++kw) {
      const int ki = ((kh * 4 + kw) * CIN + c) * 2;
      acc2 = __builtin_elementwise_fma(v2f{k[ki], k[ki + 1]}, v2f{ds[hh - kh][0][w + 3 - kw], ds[hh - kh][1][w + 3 - kw]}, acc2);
    }
  return acc2.x + acc2.y;
}

// A triple's d2 strip as the backward sees it.  The strip is the backward's own (nothing else points into it), and saying so
// lets the compiler keep the c1 taps that the forward's conv2 has just read in registers for the conv2 parameter gradients
// instead of reading them from LDS again between the `park` atomics (the phases are optimised one by one before they are
// inlined, and without this the reuse is lost: +8 LDS reads, each behind its own wait, at one position per lane).  Only for
// the narrow groups: past three positions per lane, and for a wavefront per triple, the promise costs 35-46 registers and with
// them a wave per SIMD (or, at five positions of the fused form, scratch).
template <class S>
using D2Strip = std::conditional_t<(S::LPT < 64 && S::WPL <= 3), float (*__restrict__)[2][S::DP], float (*)[2][S::DP]>;

// backward of one triple from its dflat row `gi` (global dflat, or the block's own d1 strip: the row is taken out before the
// strip is written), after conv_forward_triple has left x / c1 in the strips and the activations in `a`
template <class S>
__device__ __forceinline__ void conv_backward_triple(const ConvParams& p, const S& sh, const ConvWeights<S::WPL>& wt, const ConvActs<S::WPL>& a,
                                                     const float* gi, int64_t t, int ra, bool live, const float (*xs)[S::DPX],
                                                     const float (*c1s)[2][S::DP], D2Strip<S> d2s, float (*d1s)[2][S::DP],
                                                     const ParamGradSlots<S>& pg, float (&a_gam)[S::WPL], float (&a_bet)[S::WPL]) {
  constexpr int WPL = S::WPL, LPT = S::LPT;
  const int d = p.dim, tl = sh.tl;
  const float bn_s = rsqrtf(1.0f + CNN_BN_EPS);
  // ---- width-normalisation backward, tanh', parameter gradients of conv2 -------------------------------
  float dy[2][2][WPL], dot[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int f = 0; f < 2; ++f) dot[h][f] = 0.f;
#pragma unroll
  for (int i = 0; i < WPL; ++i) {
    const int w = tl + LPT * i;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float2 v = make_float2(0.f, 0.f);
      if (live && w < d) v = *reinterpret_cast<const float2*>(gi + h * 2 * d + w * 2);
      dy[h][0][i] = v.x; dy[h][1][i] = v.y;
#pragma unroll
      for (int f = 0; f < 2; ++f) dot[h][f] = fmaf(dy[h][f][i], a.c2[h][f][i] * a.nrm[h][f], dot[h][f]);
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int f = 0; f < 2; ++f) dot[h][f] = S::group_sum(dot[h][f]);
  float dp2[2][2][WPL];
#pragma unroll
  for (int i = 0; i < WPL; ++i) {
    const int w = tl + LPT * i;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const float y = a.c2[h][f][i] * a.nrm[h][f];
        const float dc2 = a.ssq[h][f] > MKE_L2_EPS ? a.nrm[h][f] * (dy[h][f][i] - y * dot[h][f]) : a.nrm[h][f] * dy[h][f][i];
        dp2[h][f][i] = (w < d) ? dc2 * (1.0f - a.c2[h][f][i] * a.c2[h][f][i]) : 0.f;
        d2s[h][f][w + 2] = dp2[h][f][i];  // index w+2 <-> width w
      }
  }
  // parameter gradients of conv2, one scalar at a time: db2[f] = sum dp2[.][f][.],
  // dK2[kh][kw][c][f] = sum_{h, w} dp2[h][f][w] * c1[h + kh][c][w + kw - 1]
  {
    // both filters of a tap at once (v_pk_fma_f32: the pair (dp2[.][0], dp2[.][1]) times the broadcast c1 value)
    v2f v = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < WPL; ++i) v += v2f{dp2[0][0][i], dp2[0][1][i]} + v2f{dp2[1][0][i], dp2[1][1][i]};
    pg.park(50, v.x);
    pg.park(51, v.y);
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int kw = 0; kw < 4; ++kw)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          v2f g = {0.f, 0.f};
#pragma unroll
          for (int h = 0; h + kh < 2; ++h)
#pragma unroll
            for (int i = 0; i < WPL; ++i) {
              const float x = c1s[h + kh][c][tl + LPT * i + kw];
              g = __builtin_elementwise_fma(v2f{dp2[h][0][i], dp2[h][1][i]}, v2f{x, x}, g);
            }
          pg.park(18 + ((kh * 4 + kw) * 2 + c) * 2, g.x);
          pg.park(18 + ((kh * 4 + kw) * 2 + c) * 2 + 1, g.y);
        }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int f = 0; f < 2; ++f) sh.template zero_halo<2>(d2s[h][f]);
  wave_lds_sync();
  // ---- conv2 transposed -> dc1, tanh', parameter gradients of conv1 -----------------------------------
  float dp1[2][2][WPL];
#pragma unroll
  for (int i = 0; i < WPL; ++i) {
    const int w = tl + LPT * i;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float acc = conv_transposed<2, S>(wt.k2, d2s, hh, c, w);
        dp1[hh][c][i] = (w < d) ? acc * (1.0f - a.c1[hh][c][i] * a.c1[hh][c][i]) : 0.f;
        d1s[hh][c][w + 2] = dp1[hh][c][i];
      }
  }
  // parameter gradients of conv1: db1[c], dK1[kh][kw][0][c] = sum_{h, w} dp1[h][c][w] * x[h + kh][w + kw - 1]
  {
    v2f v = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < WPL; ++i) v += v2f{dp1[0][0][i], dp1[0][1][i]} + v2f{dp1[1][0][i], dp1[1][1][i]};
    pg.park(16, v.x);
    pg.park(17, v.y);
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int kw = 0; kw < 4; ++kw) {
        v2f g = {0.f, 0.f};
#pragma unroll
        for (int hh = 0; hh + kh < 2; ++hh)
#pragma unroll
          for (int i = 0; i < WPL; ++i) {
            const float x = xs[hh + kh][tl + LPT * i + kw];
            g = __builtin_elementwise_fma(v2f{dp1[hh][0][i], dp1[hh][1][i]}, v2f{x, x}, g);
          }
        pg.park((kh * 4 + kw) * 2, g.x);
        pg.park((kh * 4 + kw) * 2 + 1, g.y);
      }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int f = 0; f < 2; ++f) sh.template zero_halo<2>(d1s[h][f]);
  wave_lds_sync();
  // ---- conv1 transposed -> dx, batch-norm affine backward, attribute-row gradient ---------------------
#pragma unroll
  for (int i = 0; i < WPL; ++i) {
    const int w = tl + LPT * i;
    float dx[2];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const float acc = conv_transposed<1, S>(wt.k1, d1s, hh, 0, w);
      dx[hh] = (live && w < d) ? acc : 0.f;
    }
    a_gam[i] += (dx[0] * a.raw[0][i] + dx[1] * a.raw[1][i]) * bn_s;
    a_bet[i] += dx[0] + dx[1];
    if (live && w < d && p.gattr) atomic_add_f32(p.gattr + (t % p.gattr_copies) * p.gattr_copy_elems + (int64_t)ra * p.attr_stride + w, dx[0] * wt.gam[i] * bn_s);
  }
  if (live && tl == 0 && p.gattr) p.tattr[ra] = p.tag;
  wave_lds_sync();
}

// ---- block-reduce the parameter gradients, one atomic per block per scalar --------------------------------
// the 16 quarter-wave slots of every scalar were filled during the loop (`park`); 52 threads add them up.  (First
// version: 52 full wave reductions + LDS atomics per wave = 20 of the kernel's 45 us.)  gamma / beta are per width
// position: the four waves' vectors go through the (now free) x / c1 strips `gsum` / `bsum`.
template <class S>
__device__ __forceinline__ void conv_reduce_param_grads(const ConvParams& p, const S& sh, const ParamGradSlots<S>& pg, const float (&a_gam)[S::WPL],
                                                        const float (&a_bet)[S::WPL], float* gsum, float* bsum) {
  constexpr int WPL = S::WPL, LPT = S::LPT;
  const int d = p.dim;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < WPL; ++i) {
    gsum[sh.slot * LPT * WPL + sh.tl + LPT * i] = a_gam[i];
    bsum[sh.slot * LPT * WPL + sh.tl + LPT * i] = a_bet[i];
  }
  __syncthreads();
  // Every block adding its 2d + 52 sums straight into grad_params is a chain of gridDim.x same-address atomics per
  // scalar (measured: 45 of the kernel's 66 us at 1024 blocks).  With a workspace the blocks spread over
  // CNN_WS_COPIES privatised copies (chain length gridDim.x / copies); whoever consumes the gradient next (the dense
  // update, or k_cnn_ws_fold) adds the copies up and zeroes them.  (A last-block-done ticket was tried first: the
  // ticket is itself a gridDim.x-long same-address chain and cost more than it saved, 95 us.)
  float* dst = p.ws ? p.ws + (size_t)(blockIdx.x % CNN_WS_COPIES) * CNN_WS_STRIDE(d) : p.gparams;
  for (int w = threadIdx.x; w < d; w += S::NT) {
    float g = 0.f, b = 0.f;
#pragma unroll
    for (int k = 0; k < S::NSLOT; ++k) { g += gsum[k * LPT * WPL + w]; b += bsum[k * LPT * WPL + w]; }
    atomic_add_f32(dst + w, g);
    atomic_add_f32(dst + d + w, b);
  }
  if (threadIdx.x < CNN_NCONV) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 4 * S::NW; ++k) v += pg.part[threadIdx.x][k];
    atomic_add_f32(dst + 2 * d + threadIdx.x, v);
  }
}

// ---- the two 16-row MFMA tiles (LPT = 16: the block's 16 triples are the rows of one 16 x 16 x 4 f32 tile) ----------------
// Lane (r16, kq) holds k-steps k0 + 4 i of row r16 of A (read from `a_row`) and of NCT column tiles of B.  All of the
// wavefront's A operands out of LDS first, unconditionally from clamped columns (a guarded read compiles to an
// exec-masked branch + a full LDS wait in front of EVERY k-step's five MFMAs: 21 exposed LDS round trips, ~2,300 of the
// dense phase's 5,800 cycles; s_memtime stamps, tools/attr_stamps.py), then the MFMAs back to back; a k-step at or past
// `klim` gets a = 0, so whatever b holds there multiplies to nothing.
template <int KS, int NCT>
__device__ __forceinline__ void mfma_rows16(const float* a_row, int k0, int klim, const float (&b)[KS][NCT], f32x4 (&acc)[NCT]) {
#pragma unroll
  for (int c = 0; c < NCT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  float av[KS];
#pragma unroll
  for (int i = 0; i < KS; ++i) av[i] = a_row[min(k0 + 4 * i, klim - 1)];
#pragma unroll
  for (int i = 0; i < KS; ++i) {
    const float ai = (k0 + 4 * i < klim) ? av[i] : 0.f;
#pragma unroll
    for (int c = 0; c < NCT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai, b[i][c], acc[c], 0, 0, 0);
  }
}

// The dense layer in the forward's block — flat rows stay in LDS as the A operand of z = tanh([flat, 1] W) (dim <= 80: five
// column tiles, K = 4 dim + 1 <= 321 split over the four wavefronts as in k_gemm_tall); flat still goes to memory once (the
// weight-gradient product reads it).
struct DenseTile {
  static constexpr int KS = 21;    // k-steps of 4 per wavefront (K <= 336)
  static constexpr int NCT = 5;    // column tiles of 16
  typedef float Acc[MKE_BLOCK / 64][NCT][4][64];
};

// W fragments requested before the convolution starts
__device__ __forceinline__ void dense_prefetch(const DenseExtra& e, int d, float (&wfrag)[DenseTile::KS][DenseTile::NCT]) {
  constexpr int KS = DenseTile::KS, NCT = DenseTile::NCT;
  const int r16 = threadIdx.x & 15, kq = (threadIdx.x & 63) >> 4, wvv = threadIdx.x >> 6;
  const int K = 4 * d + 1;
#pragma unroll
  for (int i = 0; i < KS; ++i) {
    const float* __restrict__ bp = e.W + (int64_t)min(4 * KS * wvv + kq + 4 * i, K - 1) * d;
#pragma unroll
    for (int c = 0; c < NCT; ++c) wfrag[i][c] = bp[min(16 * c + r16, d - 1)];
  }
}

// ---- z tile = tanh([flat, 1] W): the block's 16 flat rows (LDS, row stride FS) x W [K][d], K split over the four wavefronts ----
template <int FS>
__device__ __forceinline__ void dense_finish(const DenseExtra& e, int d, int64_t n, const float (*s_flat)[FS],
                                             const float (&wfrag)[DenseTile::KS][DenseTile::NCT], DenseTile::Acc& s_acc) {
  constexpr int KS = DenseTile::KS, NCT = DenseTile::NCT;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  f32x4 acc[NCT];
  mfma_rows16<KS, NCT>(s_flat[r16], 4 * KS * wv + kq, 4 * d + 1, wfrag, acc);
#pragma unroll
  for (int c = 0; c < NCT; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) s_acc[wv][c][r][lane] = acc[c][r];
  __syncthreads();
  // wave w finishes column tiles w, w + 4: C/D map of the 16x16 forms: col = lane & 15, row = 4 * (lane >> 4) + reg
  float ssq = 0.f;
  const int64_t m0 = (int64_t)blockIdx.x * 16;
  for (int c = wv; c < NCT; c += MKE_BLOCK / 64) {
    const int col = 16 * c + r16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = s_acc[0][c][r][lane] + s_acc[1][c][r][lane] + s_acc[2][c][r][lane] + s_acc[3][c][r][lane];
      const int64_t orow = m0 + 4 * kq + r;
      if (col < d && orow < n) {
        v = tanh_f(v);
        e.z[orow * d + col] = v;
        ssq = fmaf(v, v, ssq);
      }
    }
  }
  // <= 8 squares per lane: 16-lane rows in f32 on DPP, the block's 16 row sums in double (block_sum_double's six 64-bit
  // shuffle steps were 1,900 cycles at the very end of the launch's critical path)
  __shared__ double s_rows[MKE_BLOCK / 16];
  ssq = sub16_sum(ssq);
  if ((threadIdx.x & 15) == 0) s_rows[threadIdx.x >> 4] = (double)ssq;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
#pragma unroll
    for (int k = 0; k < MKE_BLOCK / 16; ++k) tot += s_rows[k];
    e.ssq[blockIdx.x] = tot;
    for (int k = blockIdx.x + gridDim.x; k < MKE_LOSS_PARTIALS; k += gridDim.x) e.ssq[k] = 0.0;
  }
}

// ---- dflat rows of the block's 16 triples: [16 x dim] (dz) x [dim x 4 dim] (W^T), f32 MFMA 16x16x4 (K = dim <= 80: 20 k-steps;
// 4 dim <= 320 columns: five 16-column tiles per wavefront, no exchange between the wavefronts), straight into the d1 strips of
// the block's 16 triples (row stride `row_floats`; a triple's 4 dim values fit its own strip, which the backward only writes after
// it has taken them out), so dflat never goes to memory and the product needs no blocks of its own.  `s_dz`: the (still unused)
// x strips, NEL = dz elements per thread.
template <int NEL>
__device__ __forceinline__ void dflat_tile(const FusedExtra& e, int d, int64_t n, float* s_dz, float* s_d1, int row_floats) {
  constexpr int KSB = 20, NTB = 5;             // k-steps of 4 (dim <= 80), column tiles per wavefront (4 dim <= 320 = 20 tiles)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * 16;
  const int ncol = 4 * d;
  // B = W^T [dim][4 dim]: lane (r16, kq) of k-step i reads wt[4 i + kq][16 ct + r16]
  // — a quarter-wave reads 16 consecutive floats (from W itself the same operand is 16 rows 300 bytes apart: 16 cache lines per
  // load instead of 1, and the phase took 14 us instead of 3).  A = the block's 16 rows of dz: 1200 consecutive floats, copied
  // into the x strips with coalesced loads and read back per lane.
  float bw[KSB][NTB];
#pragma unroll
  for (int i = 0; i < KSB; ++i) {
    const int kc = min(4 * i + kq, d - 1);       // unconditional loads from clamped addresses; k >= dim contributes a = 0
#pragma unroll
    for (int c = 0; c < NTB; ++c) bw[i][c] = e.wt[kc * ncol + min(16 * (wv + 4 * c) + r16, ncol - 1)];
  }
  // row stride of the tile in LDS: odd (dim 64 with stride 64 put the 16 rows of a fragment read on ONE bank: 62.5 us per
  // step against 52.3 at dim 75)
  const int sd = d | 1;
  {
    // the tile's g and z are requested before the two batch-wide sums are added up (one round trip for all of it)
    const int64_t e0 = m0 * d, e_end = min(n, m0 + 16) * d;
    float gv[NEL], zv[NEL];
#pragma unroll
    for (int q = 0; q < NEL; ++q) {
      const int64_t el = e0 + threadIdx.x + q * MKE_BLOCK;
      const bool ok = threadIdx.x + q * MKE_BLOCK < 16 * d && el < e_end;
      gv[q] = ok ? e.dz[el] : 0.f;
      zv[q] = ok ? e.zmat[el] : 0.f;
    }
    float inv, coef;
    batch_scalars(e.ssq, e.dotp, inv, coef);
#pragma unroll
    for (int q = 0; q < NEL; ++q) {
      const int el = threadIdx.x + q * MKE_BLOCK;
      if (el < 16 * d) s_dz[(el / d) * sd + el % d] = dz_of(gv[q], zv[q], inv, coef);   // rows past n are zero in the tile
    }
  }
  __syncthreads();
  f32x4 acc[NTB];
  mfma_rows16<KSB, NTB>(s_dz + r16 * sd, kq, d, bw, acc);
  // C/D map of the 16x16 forms: col = lane & 15, row = 4 * (lane >> 4) + reg  ->  triple slot = row, dflat column = col
#pragma unroll
  for (int c = 0; c < NTB; ++c) {
    const int col = 16 * (wv + 4 * c) + r16;
    if (col < ncol) {
#pragma unroll
      for (int r = 0; r < 4; ++r) s_d1[(4 * kq + r) * row_floats + col] = acc[c][r];
    }
  }
  __syncthreads();
}

}  // namespace mke
