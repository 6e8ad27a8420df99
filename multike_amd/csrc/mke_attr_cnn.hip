// mke_attr_cnn.hip — the attribute-view CNN scorer (code/MultiKE_model.py:34-63 `conv`) for gfx950.
//
// TF1 semantics restated: stack (attribute row, literal row) -> [2, d, 1]; batch-norm in
// inference mode along the width axis (gamma[w] * x / sqrt(1 + 1e-3) + beta[w]); two conv2d(2 filters, 2x4, SAME,
// tanh); l2-normalise over the width axis per (row, channel); flatten (index h*2d + w*2 + c); dense 4d -> d with
// tanh; l2-normalise over the WHOLE [B, d] batch; score = -||h - out||^2; loss = scale * sum w * log(1 + exp(-score)).
//
// The conv stack runs in four kernels, each a short composition of the phases in mke_attr_conv.h:
//   k_attr_conv_fwd<WPL>            a wavefront per triple; flat to memory (the standalone op, and the step past dim 80)
//   k_attr_conv_fwd_dense<WPL>      a quarter-wave per triple, 16 triples per block; the dense layer z = tanh([flat, 1] W) and the
//                                   per-block sums of z^2 follow in the same block (the step up to dim 80)
//   k_attr_conv_bwd<WPL, LPT, NW>   dflat from memory: two triples per wavefront in blocks of two wavefronts up to dim 96, a
//                                   wavefront per triple past it
//   k_attr_conv_bwd_fused<WPL>      a quarter-wave per triple; the block forms its 16 rows of dflat = dz W^T itself and the
//                                   weight-gradient product rides on extra blocks of the grid (the step up to dim 80)
// The batch-global normalisation needs two batch-wide sums (sum z^2, sum g.z): kernels write per-block partials
// and the next kernel's blocks add them up themselves — no extra reduction launches, no host round trip.
#include "mke_attr_conv.h"

namespace mke {

// ---- the four convolution kernels ------------------------------------------------------------------------------------
// Common to all: each of a block's NSLOT triples has its own LDS strips, x [2][DPX] and c1 [2][2][DP] (the backward: c1 / d2 /
// d1); the triple loop has a block-uniform trip count (barriers after it).

template <int WPL>
__global__ __launch_bounds__(MKE_BLOCK, 1) void k_attr_conv_fwd(const ConvParams p) {
  using S = ConvShape<WPL, 64, MKE_BLOCK / 64>;
  __shared__ float s_x[S::NSLOT][2][S::DPX];
  __shared__ float s_c1[S::NSLOT][2][2][S::DP];
  const S sh;
  ConvWeights<WPL> wt;
  wt.template load<S::LPT>(p.params, p.dim, sh.tl);
  const int64_t per_pass = (int64_t)gridDim.x * S::NSLOT, iters = (p.n + per_pass - 1) / per_pass;
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t t = sh.first_triple() + it * per_pass;
    const bool live = t < p.n;
    const int ra = live ? p.ia[t] : 0, rv = live ? p.iv[t] : 0;
    ConvActs<WPL> a;
    conv_forward_triple(p, sh, wt, ra, rv, live, s_x[sh.slot], s_c1[sh.slot], a);
    conv_store_flat<false>(p, sh, a, t, live, nullptr);
    wave_lds_sync();  // LDS strips are rewritten by the next iteration
  }
  __syncthreads();
}

template <int WPL>
__global__ __launch_bounds__(MKE_BLOCK, 1) void k_attr_conv_fwd_dense(const ConvParams p, const DenseExtra e) {
  using S = ConvShape<WPL, 16, MKE_BLOCK / 64>;
  constexpr int FS = 4 * S::LPT * WPL + 5;         // row stride of the flat tile (odd: conflict-free column reads)
  __shared__ float s_flat[S::NSLOT][FS];
  __shared__ DenseTile::Acc s_acc;
  __shared__ float s_x[S::NSLOT][2][S::DPX];
  __shared__ float s_c1[S::NSLOT][2][2][S::DP];
  float wfrag[DenseTile::KS][DenseTile::NCT];
  dense_prefetch(e, p.dim, wfrag);
  const S sh;
  ConvWeights<WPL> wt;
  wt.template load<S::LPT>(p.params, p.dim, sh.tl);
  const int64_t per_pass = (int64_t)gridDim.x * S::NSLOT, iters = (p.n + per_pass - 1) / per_pass;
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t t = sh.first_triple() + it * per_pass;
    const bool live = t < p.n;
    const int ra = live ? p.ia[t] : 0, rv = live ? p.iv[t] : 0;
    ConvActs<WPL> a;
    conv_forward_triple(p, sh, wt, ra, rv, live, s_x[sh.slot], s_c1[sh.slot], a);
    conv_store_flat<true>(p, sh, a, t, live, s_flat[sh.slot]);
    wave_lds_sync();  // LDS strips are rewritten by the next iteration
  }
  __syncthreads();  // every wavefront reads all 16 rows of the flat tile
  dense_finish<FS>(e, p.dim, p.n, s_flat, wfrag, s_acc);
}

template <int WPL, int LPT, int NW>
__global__ __launch_bounds__(NW * 64, 1) void k_attr_conv_bwd(const ConvParams p) {
  using S = ConvShape<WPL, LPT, NW>;
  __shared__ float s_x[S::NSLOT][2][S::DPX];
  __shared__ float s_strips[3][S::NSLOT][2][2][S::DP];   // c1 / d2 / d1
  __shared__ typename ParamGradSlots<S>::Part s_part;
  const S sh;
  ConvWeights<WPL> wt;
  wt.template load<LPT>(p.params, p.dim, sh.tl);
  const ParamGradSlots<S> pg(s_part, sh);
  float a_gam[WPL] = {}, a_bet[WPL] = {};
  const int64_t per_pass = (int64_t)gridDim.x * S::NSLOT, iters = (p.n + per_pass - 1) / per_pass;
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t t = sh.first_triple() + it * per_pass;
    const bool live = t < p.n;
    const int ra = live ? p.ia[t] : 0, rv = live ? p.iv[t] : 0;
    ConvActs<WPL> a;
    conv_forward_triple(p, sh, wt, ra, rv, live, s_x[sh.slot], s_strips[0][sh.slot], a);
    conv_backward_triple(p, sh, wt, a, p.dflat + t * (int64_t)(4 * p.dim), t, ra, live, s_x[sh.slot], s_strips[0][sh.slot],
                         s_strips[1][sh.slot], s_strips[2][sh.slot], pg, a_gam, a_bet);
  }
  __syncthreads();  // the strips are reused by the block-level reduction
  conv_reduce_param_grads(p, sh, pg, a_gam, a_bet, &s_x[0][0][0], &s_strips[0][0][0][0][0]);
}

// Round 4: the forward's shape (a quarter-wave per triple, four wavefronts).  The block first computes ITS 16 rows of dflat = dz W^T
// on the matrix cores straight into the d1 strips of its 16 triples (dflat_tile); the weight-gradient product rides on extra blocks
// at the END of the grid (dispatched after the convolution blocks, which are the long ones).
template <int WPL>
__global__ __launch_bounds__(MKE_BLOCK, 2) void k_attr_conv_bwd_fused(const ConvParams p, const FusedExtra e) {
  using S = ConvShape<WPL, 16, MKE_BLOCK / 64>;
  __shared__ float s_x[S::NSLOT][2][S::DPX];
  // the c1 / d2 / d1 strips as ONE array: the rider blocks' exchange area (20 KB) is aliased onto its start whatever the width
  // (aliased onto the c1 strips alone it fitted only above dim 64, and at dim 64 itself the block then took 82 KB of LDS = one
  // per compute unit: 62 us per step against 52 at dim 75)
  __shared__ union {
    float strips[3][S::NSLOT][2][2][S::DP];
    float rider[MKE_BLOCK / 64][5][4][64];
  } s;
  __shared__ typename ParamGradSlots<S>::Part s_part;
  static_assert(2 * 2 * S::DP >= 4 * S::LPT * WPL, "a triple's dflat row must fit its own d1 strip");
  static_assert(sizeof(s_x) >= sizeof(float) * S::NSLOT * (S::LPT * WPL + 1), "the dz tile (16 rows of dim <= 16 WPL floats, odd row stride) must fit the x strips");
  if ((int)blockIdx.x >= e.conv_blocks) {      // block-uniform: a rider of the weight-gradient product
    const int r = (int)blockIdx.x - e.conv_blocks;
    float inv, coef;
    batch_scalars(e.ssq, e.dotp, inv, coef);
    gemm_tall_block_dz<5, 32, 4>(e.tall, r % e.tall.gx, r / e.tall.gx, s.rider, e.zmat, inv, coef);
    return;
  }
  const S sh;
  // BEFORE the convolution's constants are loaded: the 100 B fragments and the 50 filter weights are never live together
  // (together: 256 registers and 232 spilled).  The host launches one block per 16 triples (a single pass of the loop below).
  dflat_tile<(S::NSLOT * S::LPT * WPL + S::NT - 1) / S::NT>(e, p.dim, p.n, &s_x[0][0][0], &s.strips[2][0][0][0][0], 2 * 2 * S::DP);
  ConvWeights<WPL> wt;
  wt.template load<S::LPT>(p.params, p.dim, sh.tl);
  const ParamGradSlots<S> pg(s_part, sh);
  float a_gam[WPL] = {}, a_bet[WPL] = {};
  const int64_t per_pass = (int64_t)e.conv_blocks * S::NSLOT, iters = (p.n + per_pass - 1) / per_pass;
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t t = sh.first_triple() + it * per_pass;
    const bool live = t < p.n;
    const int ra = live ? p.ia[t] : 0, rv = live ? p.iv[t] : 0;
    ConvActs<WPL> a;
    conv_forward_triple(p, sh, wt, ra, rv, live, s_x[sh.slot], s.strips[0][sh.slot], a);
    conv_backward_triple(p, sh, wt, a, &s.strips[2][sh.slot][0][0][0], t, ra, live, s_x[sh.slot], s.strips[0][sh.slot],
                         s.strips[1][sh.slot], s.strips[2][sh.slot], pg, a_gam, a_bet);
  }
  __syncthreads();  // the strips are reused by the block-level reduction
  conv_reduce_param_grads(p, sh, pg, a_gam, a_bet, &s_x[0][0][0], &s.strips[0][0][0][0][0]);
}

// grad_params[i] += sum over the CNN_WS_COPIES privatised copies, copies zeroed (the standalone entry's epilogue; inside
// mke_attr_step the dense update does this itself)
__global__ __launch_bounds__(MKE_BLOCK) void k_cnn_ws_fold(float* __restrict__ ws, float* __restrict__ gparams, int np, int stride) {
  const int i = blockIdx.x * MKE_BLOCK + threadIdx.x;
  if (i >= np) return;
  float v = 0.f;
#pragma unroll 8
  for (int c = 0; c < CNN_WS_COPIES; ++c) v += ws[(size_t)c * stride + i];
  for (int c = 0; c < CNN_WS_COPIES; ++c) ws[(size_t)c * stride + i] = 0.f;
  gparams[i] += v;
}

// ---- tail: z = tanh(zpre + bias), partial sums of z^2 -------------------------------------------------------------
__global__ __launch_bounds__(MKE_BLOCK) void k_attr_tail_z(float* __restrict__ z, const float* __restrict__ bias, int64_t n,
                                                           int dim, double* __restrict__ partials) {
  const int64_t total = n * dim;
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * MKE_BLOCK) {
    const float v = tanhf(bias ? z[i] + bias[i % dim] : z[i]);
    z[i] = v;
    s = fmaf(v, v, s);
  }
  const double tot = block_sum_double(s);
  if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

struct TailParams {
  const float* __restrict__ z;
  const double* __restrict__ sumsq;
  const float* __restrict__ ent;
  int ent_stride, ent_norm;
  const int32_t* __restrict__ ih;
  const float* __restrict__ ws;
  float scale;
  int64_t n;
  int dim;
  float* __restrict__ gout;
  double* __restrict__ dotp;
  float* __restrict__ gent;
  int32_t* __restrict__ tent;
  int32_t tag;
  double* __restrict__ lossp;
  const float* __restrict__ w;   // nullable pair: side job wt[k][f] = w[f][k], f < 4 dim, k < dim (the dense layer's weights transposed,
  float* __restrict__ wt;        // for the dflat product inside the convolution-backward launch)
};

template <int FPL>
__global__ __launch_bounds__(MKE_BLOCK) void k_attr_tail_loss(const TailParams p) {
  if (p.wt) {
    const int total_w = 4 * p.dim * p.dim;
    for (int e = blockIdx.x * MKE_BLOCK + threadIdx.x; e < total_w; e += gridDim.x * MKE_BLOCK) {
      const int k = e / (4 * p.dim), f = e - k * (4 * p.dim);
      p.wt[e] = p.w[f * p.dim + k];
    }
  }
  const int j = threadIdx.x & 15;
  const int64_t sub0 = ((int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x) >> 4;
  const int64_t nsub = ((int64_t)gridDim.x * MKE_BLOCK) >> 4;
  // a row's id, z values and weight are requested one row ahead — the first row's before the partial sums are added up, so
  // that its memory round trip and theirs are the same one
  int row_n = 0;
  float Zn[FPL], w_n = 1.0f;
  auto request = [&](int64_t i) {
    const bool ok = i < p.n;
    row_n = ok ? p.ih[i] : 0;
    w_n = (ok && p.ws) ? p.ws[i] : 1.0f;
    const float* zp = p.z + (ok ? i : 0) * (int64_t)p.dim + j;
#pragma unroll
    for (int k = 0; k < FPL; ++k) Zn[k] = (ok && k * 16 + j < p.dim) ? zp[k * 16] : 0.f;
  };
  request(sub0);
  const double S = total_of_partials(p.sumsq);
  const float inv = rsqrtf(fmaxf((float)S, MKE_L2_EPS));
  float loss = 0.f, dotacc = 0.f;
  for (int64_t i = sub0; i < p.n; i += nsub) {
    const int row = row_n;
    const float w = w_n;
    float H[FPL], Z[FPL];
    load_row<FPL>(p.ent, row, p.ent_stride, j, H);
#pragma unroll
    for (int k = 0; k < FPL; ++k) Z[k] = Zn[k];
    request(i + nsub);
    l2_normalize_row<FPL>(H, p.ent_norm);
    float x = 0.f;
#pragma unroll
    for (int k = 0; k < FPL; ++k) {
      H[k] = H[k] - Z[k] * inv;  // diff = h - out
      x = fmaf(H[k], H[k], x);
    }
    x = sub16_sum(x);
    loss += w * softplus_f(x);
    const float c = 2.0f * p.scale * w * sigmoid_f(x);
    float dz = 0.f;
    float* go = p.gout + i * (int64_t)p.dim + j;
#pragma unroll
    for (int k = 0; k < FPL; ++k) {
      H[k] *= c;  // g_h = 2 c diff ; g_out = -g_h
      if (k * 16 + j < p.dim) go[k * 16] = -H[k];
      dz = fmaf(-H[k], Z[k], dz);
    }
    dotacc += dz;  // per-lane partial of sum g_out . z
    if (p.gent) {
      atomic_add_row<FPL>(p.gent, row, p.ent_stride, p.dim, j, H, 1.0f);
      if (j == 0) p.tent[row] = p.tag;
    }
  }
  const double lt = block_sum_double(j == 0 ? loss : 0.f);
  __syncthreads();
  const double dt = block_sum_double(dotacc);
  if (threadIdx.x == 0) {
    p.lossp[blockIdx.x] = lt * (double)p.scale;
    p.dotp[blockIdx.x] = dt;
    // one pass over the rows takes n / 16 blocks; the partial slots no block owns are cleared here (every block of this and
    // of the next kernel re-adds all MKE_LOSS_PARTIALS slots: 2048 blocks doing that was 32 MB of L2 reads)
    for (int k = blockIdx.x + gridDim.x; k < MKE_LOSS_PARTIALS; k += gridDim.x) { p.lossp[k] = 0.0; p.dotp[k] = 0.0; }
  }
}

// dzpre = inv * (g_out - out * (g_out . out)) * (1 - z^2), in place over gout
__global__ __launch_bounds__(MKE_BLOCK) void k_attr_tail_bwd(const float* __restrict__ z, float* __restrict__ g,
                                                             const double* __restrict__ sumsq, const double* __restrict__ dotp,
                                                             int64_t n, int dim) {
  // the first four elements of every thread (all of them when the grid is sized by the launcher) are requested before the
  // partial sums: one memory round trip in front of the arithmetic instead of three
  const int64_t total = n * dim;
  const int64_t i0 = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x, step = (int64_t)gridDim.x * MKE_BLOCK;
  float zv[4], gv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t i = i0 + j * step;
    zv[j] = i < total ? z[i] : 0.f;
    gv[j] = i < total ? g[i] : 0.f;
  }
  float inv, coef;
  batch_scalars(sumsq, dotp, inv, coef);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t i = i0 + j * step;
    if (i < total) g[i] = inv * (gv[j] - zv[j] * coef) * (1.0f - zv[j] * zv[j]);
  }
  for (int64_t i = i0 + 4 * step; i < total; i += step) {
    const float zz = z[i];
    g[i] = inv * (g[i] - zz * coef) * (1.0f - zz * zz);
  }
}

// out[j] += sum_i x[i][j]: each block folds its rows, one atomic per column per block (standalone bias gradient; inside
// mke_attr_step the bias is a row of the extended weight matrix and its gradient a row of dW)
__global__ __launch_bounds__(MKE_BLOCK) void k_colsum_add(const float* __restrict__ x, int64_t n, int dim, float* __restrict__ out) {
  for (int j = threadIdx.x; j < dim; j += MKE_BLOCK) {
    float s = 0.f;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) s += x[i * dim + j];
    atomic_add_f32(out + j, s);
  }
}

__global__ __launch_bounds__(MKE_BLOCK) void k_dense_update(const DenseJob j) { dense_update_range(j, blockIdx.x, gridDim.x); }

// ---- host side ---------------------------------------------------------------------------------------------------------

// Dispatch a kernel template on WPL = width positions per lane (1..5).
#define MKE_DISPATCH_WPL(wpl, dim, ...)                                               \
  switch (wpl) {                                                                      \
    case 1: { constexpr int WPL = 1; __VA_ARGS__; } break;                            \
    case 2: { constexpr int WPL = 2; __VA_ARGS__; } break;                            \
    case 3: { constexpr int WPL = 3; __VA_ARGS__; } break;                            \
    case 4: { constexpr int WPL = 4; __VA_ARGS__; } break;                            \
    case 5: { constexpr int WPL = 5; __VA_ARGS__; } break;                            \
    default:                                                                          \
      set_error("attribute CNN: dim %d not supported (<= 320)", dim);                 \
      return MKE_E_UNSUPPORTED;                                                       \
  }

// the gather side of every convolution launch; the caller adds the outputs of its direction
static ConvParams make_conv_params(const float* attr, int attr_stride, int attr_norm, const float* lit, int lit_stride, int dim,
                                   const int32_t* ia, const int32_t* iv, int64_t n, const float* params) {
  ConvParams p{};
  p.attr = attr; p.attr_stride = attr_stride; p.attr_norm = attr_norm; p.lit = lit; p.lit_stride = lit_stride;
  p.dim = dim; p.ia = ia; p.iv = iv; p.n = n; p.params = params;
  return p;
}

static unsigned conv_blocks_capped(int64_t n, int per_block) {
  int64_t blocks = (n + per_block - 1) / per_block;
  if (blocks > 4096) blocks = 4096;  // one triple per group up to 16K (32K) triples: no half-idle second pass
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

// a wavefront per triple (the forward is a latency chain and prefers twice the wavefronts of the two-triples form)
static int launch_conv_fwd(const ConvParams& p, hipStream_t st) {
  const unsigned nb = conv_blocks_capped(p.n, MKE_BLOCK / 64);
  MKE_DISPATCH_WPL((p.dim + 63) / 64, p.dim, { hipLaunchKernelGGL((k_attr_conv_fwd<WPL>), dim3(nb), dim3(MKE_BLOCK), 0, st, p); });
  return check_launch("k_attr_conv_fwd");
}

// conv stack + dense layer, 16 triples per block (the caller checked dim <= 80, n <= 16 MKE_LOSS_PARTIALS)
static int launch_conv_fwd_dense(const ConvParams& p, const DenseExtra& e, hipStream_t st) {
  const unsigned nb = (unsigned)((p.n + 15) / 16);
  MKE_DISPATCH_WPL((p.dim + 15) / 16, p.dim, { hipLaunchKernelGGL((k_attr_conv_fwd_dense<WPL>), dim3(nb), dim3(MKE_BLOCK), 0, st, p, e); });
  return check_launch("k_attr_conv_fwd_dense");
}

// dim <= 96: two triples per wavefront, 32 lanes each (dim 75: three passes of 32 lanes instead of two of 64), in blocks of two
// wavefronts (the backward is bound by instruction issue)
static int launch_conv_bwd(const ConvParams& p, hipStream_t st) {
  if (p.dim <= 96) {
    const unsigned nb = conv_blocks_capped(p.n, 4);
    MKE_DISPATCH_WPL((p.dim + 31) / 32, p.dim, {
      if constexpr (WPL <= 3) hipLaunchKernelGGL((k_attr_conv_bwd<WPL, 32, 2>), dim3(nb), dim3(128), 0, st, p);
      else { set_error("attribute CNN: dim %d not supported", p.dim); return MKE_E_UNSUPPORTED; }
    });
  } else {
    const unsigned nb = conv_blocks_capped(p.n, MKE_BLOCK / 64);
    MKE_DISPATCH_WPL((p.dim + 63) / 64, p.dim, {
      if constexpr (WPL >= 2) hipLaunchKernelGGL((k_attr_conv_bwd<WPL, 64, MKE_BLOCK / 64>), dim3(nb), dim3(MKE_BLOCK), 0, st, p);
      else { set_error("attribute CNN: dim %d not supported (<= 320)", p.dim); return MKE_E_UNSUPPORTED; }
    });
  }
  return check_launch("k_attr_conv_bwd");
}

// the backward with its dflat rows computed in the block and the weight-gradient product on rider blocks (dim <= 80)
static int launch_conv_bwd_fused(const ConvParams& p, const FusedExtra& e, hipStream_t st) {
  const unsigned nb = (unsigned)e.conv_blocks + (unsigned)(e.tall.gx * e.tall.gz);
  MKE_DISPATCH_WPL((p.dim + 15) / 16, p.dim, { hipLaunchKernelGGL((k_attr_conv_bwd_fused<WPL>), dim3(nb), dim3(MKE_BLOCK), 0, st, p, e); });
  return check_launch("k_attr_conv_bwd_fused");
}

static int ws_fold(float* ws, float* gparams, int dim, hipStream_t st) {
  const int np = 2 * dim + CNN_NCONV;
  hipLaunchKernelGGL(k_cnn_ws_fold, dim3((np + MKE_BLOCK - 1) / MKE_BLOCK), dim3(MKE_BLOCK), 0, st, ws, gparams, np, CNN_WS_STRIDE(dim));
  return check_launch("k_cnn_ws_fold");
}

static int dense_update_impl(float* param, float* acc, float* grad, int64_t n, int optimizer, float lr, float* ws, int ws_n,
                             int ws_stride, hipStream_t st) {
  if (n < 0) { set_error("negative n"); return MKE_E_SHAPE; }
  if (n == 0) return MKE_OK;
  if (!param || !grad) { set_error("mke_dense_update: NULL pointer"); return MKE_E_NULL; }
  if (optimizer != MKE_OPT_ADAGRAD && optimizer != MKE_OPT_SGD) { set_error("unsupported optimizer %d", optimizer); return MKE_E_UNSUPPORTED; }
  if (optimizer == MKE_OPT_ADAGRAD && !acc) { set_error("Adagrad needs an accumulator"); return MKE_E_NULL; }
  int64_t blocks = (n + MKE_BLOCK - 1) / MKE_BLOCK;
  if (blocks > 1024) blocks = 1024;
  DenseJob j{param, acc, grad, n, optimizer, lr, ws, ws_n, ws_stride, CNN_WS_COPIES};
  hipLaunchKernelGGL(k_dense_update, dim3((unsigned)blocks), dim3(MKE_BLOCK), 0, st, j);
  return check_launch("k_dense_update");
}

// w / wt: nullable pair, the side job of TailParams (the step's fused backward)
static int tail_loss_impl(const float* z, const double* sumsq_partials, const float* ent_table, int ent_stride,
                          int ent_normalize, const int32_t* ih, const float* weights, float scale, int64_t n, int dim,
                          float* gout, double* dot_partials, float* grad_ent, int32_t* touched_ent, int32_t tag,
                          double* loss_partials, const float* w, float* wt, void* stream) {
  if (n < 0 || dim <= 0 || ent_stride % 16 != 0 || dim > ent_stride || ent_stride > MKE_MAX_STRIDE) { set_error("bad n/dim/stride"); return MKE_E_SHAPE; }
  if (!z || !sumsq_partials || !ent_table || !gout || !dot_partials || !loss_partials || (n > 0 && !ih)) { set_error("mke_attr_tail_loss: NULL pointer"); return MKE_E_NULL; }
  if (grad_ent && !touched_ent) { set_error("NULL touched array"); return MKE_E_NULL; }
  TailParams p;
  p.z = z; p.sumsq = sumsq_partials; p.ent = ent_table; p.ent_stride = ent_stride; p.ent_norm = ent_normalize; p.ih = ih;
  p.ws = weights; p.scale = scale; p.n = n; p.dim = dim; p.gout = gout; p.dotp = dot_partials; p.gent = grad_ent;
  p.tent = touched_ent; p.tag = tag; p.lossp = loss_partials; p.w = w; p.wt = wt;
  const int fpl = ent_stride / 16;
  int64_t blocks = (n + MKE_SUBS_PER_BLOCK - 1) / MKE_SUBS_PER_BLOCK;
  blocks = std::max<int64_t>(1, std::min<int64_t>(blocks, MKE_LOSS_PARTIALS));
  MKE_DISPATCH_FPL(fpl, {
    hipLaunchKernelGGL((k_attr_tail_loss<FPL>), dim3((unsigned)blocks), dim3(MKE_BLOCK), 0, (hipStream_t)stream, p);
  });
  return check_launch("k_attr_tail_loss");
}

// ---- the training step, phase by phase ---------------------------------------------------------------------------------

// one step's view of its scratch and parameters
struct StepCtx {
  int d;
  int64_t n;
  int fs;                    // row stride of flat: column 4d is the constant 1 that carries the bias through the GEMMs
  float *flat, *dflat, *z, *gout;
  float *W, *gW;             // bias / its gradient are row 4d of W / gW (packed right behind)
  double *lossp, *ssq, *dot;
  bool fused_tail;           // the loss tail leaves W^T in the dflat scratch for the fused backward
  void* stream;
};

// The fused backward reads W^T from the scratch where the step's loss tail left it.  A call that runs the backward
// WITHOUT the tail (mke_attr_step_phases: the sharded view all-reduces a scalar between the two) takes the fused path only
// when the last tail enqueued on this scratch was this step's (same tag, same parameters) and did leave W^T — otherwise (the
// option toggled in between, a BWD-only call out of the blue) the unfused path, which needs nothing but g in `gout`
// (round-4 advice).  Host-side bookkeeping of what was ENQUEUED; stream order makes it true on the device.
// Per host thread (two threads driving two attribute graphs do not see each other's note: round-5 advice), single use: the
// backward that consumes it, an update of these parameters (W changes) or any other tail on this thread clears it, so a
// BWD-only call that re-uses a tag later never finds a stale W^T.
struct TransposedWeightNote {
  const float* scratch = nullptr;
  const float* params = nullptr;
  int32_t tag = 0;
  void leave(const float* s, const float* p, int32_t t) { scratch = s; params = p; tag = t; }   // s == nullptr: the tail left none
  bool consume(const float* s, const float* p, int32_t t) {   // one backward per tail
    const bool found = scratch == s && params == p && tag == t;
    scratch = nullptr;
    return found;
  }
  void invalidate(const float* p) { if (params == p) scratch = nullptr; }   // the parameters move: W^T is stale
};
static thread_local TransposedWeightNote wt_note;

static ConvParams step_conv_params(const mke_attr_step_args* a) {
  return make_conv_params(a->attr_table, a->attr_stride, a->attr_normalize, a->lit_table, a->lit_stride, a->dim, a->ia, a->iv, a->n, a->params);
}

// forward: conv stack -> dense -> tanh, per-block sums of z^2
static int step_forward(const mke_attr_step_args* a, const StepCtx& c) {
  hipStream_t st = (hipStream_t)c.stream;
  if (c.d <= 80 && (c.n + 15) / 16 <= MKE_LOSS_PARTIALS) {
    // one launch: conv stack, then z = tanh([flat, 1] [W; bias]) on the block's 16 flat rows, per-block sums of z^2
    ConvParams p = step_conv_params(a);
    p.flat = c.flat; p.flat_stride = c.fs;
    return launch_conv_fwd_dense(p, DenseExtra{c.W, c.z, c.ssq}, st);
  }
  if (int rc = mke_attr_conv_fwd(a->attr_table, a->attr_stride, a->attr_normalize, a->lit_table, a->lit_stride, c.d, a->ia, a->iv, c.n,
                                 a->params, c.flat, c.fs, c.stream)) return rc;
  // z = tanh([flat, 1] [W; bias]) with the per-block sums of z^2 written by the GEMM's epilogue
  return launch_gemm_f32(c.flat, c.fs, 1, c.W, c.d, 1, c.z, c.d, (int)c.n, c.d, 4 * c.d + 1, 1, 0, st, c.ssq, 0);
}

// batch-global normalisation -> loss, g = dL/dout in gout, per-block sums of g . z
static int step_tail(const mke_attr_step_args* a, const StepCtx& c) {
  if (int rc = tail_loss_impl(c.z, c.ssq, a->ent_table, a->ent_stride, a->ent_normalize, a->ih, a->weights, a->scale, c.n, c.d, c.gout, c.dot,
                              a->ent_grad, a->ent_touched, a->tag, c.lossp, c.fused_tail ? c.W : nullptr, c.fused_tail ? c.dflat : nullptr, c.stream)) return rc;
  wt_note.leave(c.fused_tail ? c.dflat : nullptr, a->params, a->tag);
  return MKE_OK;
}

// dim <= 80 (round 4: 64 < dim <= 80; round 5: every narrower width too): the rest of the backward is ONE launch — every convolution-backward block forms its 16 rows of
// dz = dL/dzpre from g and z with the two batch-wide sums, multiplies them with W^T on the matrix cores straight into its LDS strips
// (dflat never goes to memory), and [dW; dbias] = [flat, 1]^T dz (split over K, atomic) rides on extra blocks of the same grid,
// forming dz on the way into its MFMAs.  W^T (the B operand read 16 consecutive floats per quarter-wave) is left in the unused dflat
// scratch by the loss-tail launch.  4 launches per step: forward, loss tail, backward, updates.
static int step_backward(const mke_attr_step_args* a, const StepCtx& c, bool upd) {
  hipStream_t st = (hipStream_t)c.stream;
  const int d = c.d;
  const int64_t n = c.n;
  int rc;
  const bool left = wt_note.consume(c.dflat, a->params, a->tag);
  const bool fused = c.fused_tail && left;
  if (!fused && (rc = mke_attr_tail_bwd(c.z, c.gout, c.ssq, c.dot, n, d, nullptr, c.stream))) return rc;   // gout = dL/dzpre (the fused launch forms it on load)
  if (a->attr_grad && !a->attr_touched) { set_error("mke_attr_step: NULL touched array"); return MKE_E_NULL; }
  ConvParams p = step_conv_params(a);
  p.dflat = c.dflat; p.gparams = a->param_grads; p.gattr = a->attr_grad; p.tattr = a->attr_touched; p.tag = a->tag; p.ws = a->workspace;
  p.gattr_copies = a->attr_grad_copies > 1 ? a->attr_grad_copies : 1; p.gattr_copy_elems = a->n_attr * (int64_t)a->attr_stride;
  if (fused) {
    FusedExtra e{};
    e.dz = c.gout /* g */; e.zmat = c.z; e.ssq = c.ssq; e.dotp = c.dot; e.wt = c.dflat; e.conv_blocks = (int)((n + 15) / 16);
    GemmParams& t = e.tall;
    t.A = c.flat; t.B = c.gout; t.C = c.gW; t.M = 4 * d + 1; t.N = d; t.K = (int)n; t.a_rs = 1; t.a_cs = c.fs; t.b_rs = d; t.b_cs = 1; t.ldc = d;
    t.k_per_split = 512;   // 16 x KS(32) k per rider: 190 riders at n = 5000 — with the 313 convolution blocks they are all resident at once
    t.gx = (t.M + 15) / 16; t.gy = 1; t.gz = (t.K + t.k_per_split - 1) / t.k_per_split; t.atomic = 1;
    if ((rc = launch_conv_bwd_fused(p, e, st))) return rc;
  } else {
    // [dW; dbias] = [flat, 1]^T dz (split-K, atomic)  and  dflat = dz W^T, one launch; then the convolution backward
    if (!launch_gemm_tallsplit_plus(c.flat, 1, c.fs, c.gout, d, c.gW, d, 4 * d + 1, d, (int)n,
                                    c.gout, d, 1, c.W, 1, d, c.dflat, 4 * d, (int)n, 4 * d, d, st, &rc))
      rc = launch_gemm_f32_pair(c.flat, 1, c.fs, c.gout, d, 1, c.gW, d, 4 * d + 1, d, (int)n, 32, 1,
                                c.gout, d, 1, c.W, 1, d, c.dflat, 4 * d, (int)n, 4 * d, d, 1, 0, st);
    if (rc) return rc;
    if ((rc = launch_conv_bwd(p, st))) return rc;
  }
  if (!upd && a->workspace) return ws_fold(a->workspace, a->param_grads, d, st);   // gradients complete in param_grads
  return MKE_OK;
}

// one launch: entity rows, attribute rows, and (rider blocks) the dense update of the packed parameters, which also
// adds up the privatised copies of the conv / BN gradients
static int step_update(const mke_attr_step_args* a, const StepCtx& c) {
  const int d = c.d;
  if (a->optimizer != MKE_OPT_ADAGRAD && a->optimizer != MKE_OPT_SGD) { set_error("unsupported optimizer %d", a->optimizer); return MKE_E_UNSUPPORTED; }
  if (a->optimizer == MKE_OPT_ADAGRAD && (!a->param_acc || (a->ent_grad && !a->ent_acc) || (a->attr_grad && !a->attr_acc))) { set_error("mke_attr_step: Adagrad needs accumulators"); return MKE_E_NULL; }
  if (a->ent_stride != a->attr_stride && a->ent_grad && a->attr_grad) { set_error("mke_attr_step: entity / attribute strides differ"); return MKE_E_SHAPE; }
  mke_update_table tabs[2];
  int nt = 0;
  if (a->ent_grad) tabs[nt++] = mke_update_table{a->ent_table, a->ent_acc, a->ent_grad, a->ent_touched, a->n_ent, a->ent_normalize, 1, nullptr};
  if (a->attr_grad) tabs[nt++] = mke_update_table{a->attr_table, a->attr_acc, a->attr_grad, a->attr_touched, a->n_attr, a->attr_normalize,
                                                  a->attr_grad_copies > 1 ? a->attr_grad_copies : 1, nullptr};
  DenseJob dj{a->params, a->param_acc, a->param_grads, (int64_t)MKE_CNN_PARAMS(d), a->optimizer, a->lr, a->workspace,
              MKE_CNN_CONV_PARAMS(d), CNN_WS_STRIDE(d), CNN_WS_COPIES};
  UpdateTouchedHint hint(a->n);   // at most one head row per triple
  return launch_rows_update_multi(tabs, nt, a->tag, a->ent_grad ? a->ent_stride : a->attr_stride, d, a->optimizer, a->lr, (hipStream_t)c.stream,
                                  nullptr, &dj);
}

static int attr_step_impl(const mke_attr_step_args* a, double* lossp, double* ssq, double* dot, void* stream, int phases) {
  if (!a) { set_error("mke_attr_step: NULL args"); return MKE_E_NULL; }
  if (a->n < 0 || a->dim <= 0) { set_error("mke_attr_step: bad n/dim"); return MKE_E_SHAPE; }
  if (!a->ent_table || !a->attr_table || !a->lit_table || !a->params || !a->param_grads || !a->scratch || !a->partials) { set_error("mke_attr_step: NULL pointer"); return MKE_E_NULL; }
  if (a->n == 0 && phases == MKE_ATTR_ALL) {
    hipError_t e = hipMemsetAsync(lossp, 0, sizeof(double) * MKE_LOSS_PARTIALS, (hipStream_t)stream);
    if (e != hipSuccess) { set_error("mke_attr_step: memset failed"); return (int)e; }
    return MKE_OK;
  }
  if (a->n == 0) {  // a rank that owns none of the step's triples still takes part in the reductions: its sums are zero
    hipError_t e = hipSuccess;
    if (phases & MKE_ATTR_FWD) e = hipMemsetAsync(ssq, 0, sizeof(double) * MKE_LOSS_PARTIALS, (hipStream_t)stream);
    if (e == hipSuccess && (phases & MKE_ATTR_TAIL)) e = hipMemsetAsync(lossp, 0, sizeof(double) * MKE_LOSS_PARTIALS, (hipStream_t)stream);
    if (e == hipSuccess && (phases & MKE_ATTR_TAIL)) e = hipMemsetAsync(dot, 0, sizeof(double) * MKE_LOSS_PARTIALS, (hipStream_t)stream);
    if (e != hipSuccess) { set_error("mke_attr_step: memset failed"); return (int)e; }
    phases &= MKE_ATTR_UPD;
    if (!phases) return MKE_OK;
  }
  StepCtx c;
  c.d = a->dim; c.n = a->n; c.fs = 4 * c.d + 4;
  c.flat = a->scratch; c.dflat = c.flat + c.n * c.fs; c.z = c.dflat + c.n * 4 * c.d; c.gout = c.z + c.n * c.d;
  c.W = a->params + MKE_CNN_CONV_PARAMS(c.d); c.gW = a->param_grads + MKE_CNN_CONV_PARAMS(c.d);
  c.lossp = lossp; c.ssq = ssq; c.dot = dot; c.stream = stream;
  c.fused_tail = tune_attr_fused_bwd() && c.d <= 80 && (int64_t)c.n * c.fs < (1LL << 31) && c.n >= c.d;
  int rc;
  if ((phases & MKE_ATTR_FWD) && (rc = step_forward(a, c))) return rc;
  if ((phases & MKE_ATTR_TAIL) && (rc = step_tail(a, c))) return rc;
  if ((phases & MKE_ATTR_UPD) && !(phases & MKE_ATTR_BWD)) wt_note.invalidate(a->params);
  const bool upd = a->update != 0 && (phases & MKE_ATTR_UPD);
  if ((phases & MKE_ATTR_BWD) && (rc = step_backward(a, c, upd))) return rc;
  if (upd && (rc = step_update(a, c))) return rc;
  return MKE_OK;
}

}  // namespace mke

extern "C" int mke_attr_conv_fwd(const float* attr_table, int attr_stride, int attr_normalize, const float* lit_table,
                                 int lit_stride, int dim, const int32_t* ia, const int32_t* iv, int64_t n,
                                 const float* params, float* flat, int flat_stride, void* stream) {
  using namespace mke;
  if (n < 0 || dim <= 0 || dim > MKE_MAX_STRIDE || attr_stride < dim || lit_stride < dim) { set_error("mke_attr_conv_fwd: bad n/dim/stride"); return MKE_E_SHAPE; }
  if (n == 0) return MKE_OK;
  if (!attr_table || !lit_table || !ia || !iv || !params || !flat) { set_error("mke_attr_conv_fwd: NULL pointer"); return MKE_E_NULL; }
  if (flat_stride < 4 * dim || (flat_stride & 1)) { set_error("mke_attr_conv_fwd: flat_stride must be even and >= 4*dim"); return MKE_E_SHAPE; }
  ConvParams p = make_conv_params(attr_table, attr_stride, attr_normalize, lit_table, lit_stride, dim, ia, iv, n, params);
  p.flat = flat; p.flat_stride = flat_stride;
  return launch_conv_fwd(p, (hipStream_t)stream);
}

extern "C" int mke_attr_conv_bwd(const float* attr_table, int attr_stride, int attr_normalize, const float* lit_table,
                                 int lit_stride, int dim, const int32_t* ia, const int32_t* iv, int64_t n,
                                 const float* params, const float* dflat, float* grad_params, float* grad_attr,
                                 int32_t* touched_attr, int32_t tag, float* workspace, void* stream) {
  using namespace mke;
  if (n < 0 || dim <= 0 || dim > MKE_MAX_STRIDE || attr_stride < dim || lit_stride < dim) { set_error("mke_attr_conv_bwd: bad n/dim/stride"); return MKE_E_SHAPE; }
  if (n == 0) return MKE_OK;
  if (!attr_table || !lit_table || !ia || !iv || !params || !dflat || !grad_params) { set_error("mke_attr_conv_bwd: NULL pointer"); return MKE_E_NULL; }
  if (grad_attr && !touched_attr) { set_error("NULL touched array"); return MKE_E_NULL; }
  ConvParams p = make_conv_params(attr_table, attr_stride, attr_normalize, lit_table, lit_stride, dim, ia, iv, n, params);
  p.dflat = dflat; p.gparams = grad_params; p.gattr = grad_attr; p.gattr_copies = 1; p.gattr_copy_elems = 0; p.tattr = touched_attr;
  p.tag = tag; p.ws = workspace;
  int rc = launch_conv_bwd(p, (hipStream_t)stream);
  if (rc || !workspace) return rc;
  return ws_fold(workspace, grad_params, dim, (hipStream_t)stream);
}

extern "C" int mke_attr_tail_z(float* z, const float* bias, int64_t n, int dim, double* sumsq_partials, void* stream) {
  using namespace mke;
  if (n < 0 || dim <= 0) { set_error("bad n/dim"); return MKE_E_SHAPE; }
  if (!z || !sumsq_partials) { set_error("mke_attr_tail_z: NULL pointer"); return MKE_E_NULL; }
  hipLaunchKernelGGL(k_attr_tail_z, dim3(MKE_LOSS_PARTIALS), dim3(MKE_BLOCK), 0, (hipStream_t)stream, z, bias, n, dim,
                     sumsq_partials);
  return check_launch("k_attr_tail_z");
}

extern "C" int mke_attr_tail_loss(const float* z, const double* sumsq_partials, const float* ent_table, int ent_stride,
                                  int ent_normalize, const int32_t* ih, const float* weights, float scale, int64_t n, int dim,
                                  float* gout, double* dot_partials, float* grad_ent, int32_t* touched_ent, int32_t tag,
                                  double* loss_partials, void* stream) {
  return mke::tail_loss_impl(z, sumsq_partials, ent_table, ent_stride, ent_normalize, ih, weights, scale, n, dim, gout, dot_partials,
                             grad_ent, touched_ent, tag, loss_partials, nullptr, nullptr, stream);
}

extern "C" int mke_attr_tail_bwd(const float* z, float* gout, const double* sumsq_partials, const double* dot_partials,
                                 int64_t n, int dim, float* grad_bias, void* stream) {
  using namespace mke;
  if (n < 0 || dim <= 0) { set_error("bad n/dim"); return MKE_E_SHAPE; }
  if (n == 0) return MKE_OK;
  if (!z || !gout || !sumsq_partials || !dot_partials) { set_error("mke_attr_tail_bwd: NULL pointer"); return MKE_E_NULL; }
  int64_t blocks = (n * dim + MKE_BLOCK * 4 - 1) / (MKE_BLOCK * 4);
  blocks = std::max<int64_t>(1, std::min<int64_t>(blocks, 1024));
  hipLaunchKernelGGL(k_attr_tail_bwd, dim3((unsigned)blocks), dim3(MKE_BLOCK), 0, (hipStream_t)stream, z, gout, sumsq_partials,
                     dot_partials, n, dim);
  int rc = check_launch("k_attr_tail_bwd");
  if (rc || !grad_bias) return rc;
  hipLaunchKernelGGL(k_colsum_add, dim3(64), dim3(MKE_BLOCK), 0, (hipStream_t)stream, gout, n, dim, grad_bias);
  return check_launch("k_colsum_add");
}

extern "C" int mke_dense_update(float* param, float* acc, float* grad, int64_t n, int optimizer, float lr, void* stream) {
  return mke::dense_update_impl(param, acc, grad, n, optimizer, lr, nullptr, 0, 0, (hipStream_t)stream);
}

extern "C" int64_t mke_attr_scratch_floats(int64_t n, int dim) {
  if (n < 0 || dim <= 0) return 0;
  return n * ((int64_t)dim * 10 + 4);  // flat n*(4d+4) | dflat n*4d | z n*d | gout n*d
}

extern "C" int mke_attr_step(const mke_attr_step_args* a, void* stream) {
  mke::TuningScope scope(a ? a->tuning : nullptr);   // the arguments' knobs for the duration of this call
  if (!a) { mke::set_error("mke_attr_step: NULL args"); return MKE_E_NULL; }
  if (!a->partials) { mke::set_error("mke_attr_step: NULL pointer"); return MKE_E_NULL; }
  return mke::attr_step_impl(a, a->partials, a->partials + MKE_LOSS_PARTIALS, a->partials + 2 * MKE_LOSS_PARTIALS, stream, MKE_ATTR_ALL);
}

// The same step in phases (bit mask), for the data-parallel attribute view (multike_amd/distributed_views.py): the
// batch-wide normalisation couples the ranks through two scalars, so the caller all-reduces
//   args->partials[MKE_LOSS_PARTIALS ...)      (sum z^2)  between MKE_ATTR_FWD and MKE_ATTR_TAIL,
//   args->partials[2 MKE_LOSS_PARTIALS ...)    (sum g.z)  between MKE_ATTR_TAIL and MKE_ATTR_BWD
// (replace each array by [global sum, 0, 0, ...]: the consuming kernel adds the entries up itself), and the parameter /
// attribute-table gradients between MKE_ATTR_BWD and MKE_ATTR_UPD.
extern "C" int mke_attr_step_phases(const mke_attr_step_args* a, int phases, void* stream) {
  mke::TuningScope scope(a ? a->tuning : nullptr);   // the arguments' knobs for the duration of this call
  using namespace mke;
  if (!a) { set_error("mke_attr_step_phases: NULL args"); return MKE_E_NULL; }
  if (phases <= 0 || phases > MKE_ATTR_ALL) { set_error("mke_attr_step_phases: bad phase mask"); return MKE_E_SHAPE; }
  if (!a->partials) { set_error("mke_attr_step_phases: NULL partials"); return MKE_E_NULL; }
  return mke::attr_step_impl(a, a->partials, a->partials + MKE_LOSS_PARTIALS, a->partials + 2 * MKE_LOSS_PARTIALS, stream, phases);
}

extern "C" int mke_attr_steps(const mke_attr_step_args* args, const int64_t* step_off, int n_steps, double* loss_ring, int ring,
                              void* stream) {
  mke::TuningScope scope(args ? args->tuning : nullptr);   // the arguments' knobs for the duration of this call
  using namespace mke;
  if (!args || !step_off || !loss_ring) { set_error("mke_attr_steps: NULL pointer"); return MKE_E_NULL; }
  if (n_steps < 0 || ring < 1) { set_error("mke_attr_steps: bad n_steps/ring"); return MKE_E_SHAPE; }
  if (!args->partials || !args->ih || !args->ia || !args->iv) { set_error("mke_attr_steps: NULL pointer in args"); return MKE_E_NULL; }
  if ((int64_t)args->tag + n_steps >= 0x7FFFFFFFLL) { set_error("tag overflow"); return MKE_E_RANGE; }
  for (int s = 0; s < n_steps; ++s) {
    const int64_t lo = step_off[s], hi = step_off[s + 1];
    if (lo < 0 || hi < lo) { set_error("mke_attr_steps: step_off must be non-decreasing"); return MKE_E_SHAPE; }
    mke_attr_step_args a = *args;
    a.ih += lo; a.ia += lo; a.iv += lo;
    if (a.weights) a.weights += lo;
    a.n = hi - lo;
    a.tag = args->tag + s;
    const int rc = mke::attr_step_impl(&a, loss_ring + (int64_t)(s % ring) * MKE_LOSS_PARTIALS, args->partials + MKE_LOSS_PARTIALS,
                                  args->partials + 2 * MKE_LOSS_PARTIALS, stream, MKE_ATTR_ALL);
    if (rc) return rc;
  }
  return MKE_OK;
}
