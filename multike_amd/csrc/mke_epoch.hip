// mke_epoch.hip — the relation view's epoch boundary on device: random.shuffle of both positive lists
// (code/MultiKE_model.py:314-315) and the step-contiguous layout of the new epoch's positives
// (code/base/batch.py:36-54: step s takes list positions [s*b1, (s+1)*b1) of KG 1 and [s*b2, (s+1)*b2) of KG 2, short or
// empty at the lists' ends) in ONE launch: thread i reads row perm[i] of its KG's current list once and writes it to the
// shuffled list (position i: what the next epoch's permutation composes with) and to the epoch position of list position i.
#include "mke_common.h"

namespace mke {

struct EpochParams {
  const int32_t* __restrict__ list_in[2];   // [n][3] (h, r, t)
  int32_t* __restrict__ list_out[2];        // nullable
  const int64_t* __restrict__ perm[2];      // nullable = identity
  int64_t n[2];
  int64_t b[2];                             // list positions of the KG per step
  int64_t n_steps;
  int32_t* __restrict__ pos_h;
  int32_t* __restrict__ pos_r;
  int32_t* __restrict__ pos_t;
};

__global__ __launch_bounds__(MKE_BLOCK) void k_epoch_positives(const EpochParams p) {
  int64_t i = (int64_t)blockIdx.x * MKE_BLOCK + threadIdx.x;
  int kg = 0;
  if (i >= p.n[0]) { i -= p.n[0]; kg = 1; }
  if (i >= p.n[kg]) return;
  const int64_t src = p.perm[kg] ? p.perm[kg][i] : i;
  const int32_t* row = p.list_in[kg] + 3 * src;
  const int32_t h = row[0], r = row[1], t = row[2];
  if (p.list_out[kg]) {
    int32_t* o = p.list_out[kg] + 3 * i;
    o[0] = h; o[1] = r; o[2] = t;
  }
  const int64_t b = p.b[kg];
  if (b <= 0) return;                       // this KG has no share of a step: its triples are never batched
  const int64_t s = i / b;
  if (s >= p.n_steps) return;               // past the last step (the split rounds KG 1's share down)
  // steps before s took min(s*b1, n1) + min(s*b2, n2) positives; inside step s the KG 1 part comes first
  const int64_t before1 = min(s * p.b[0], p.n[0]), before2 = min(s * p.b[1], p.n[1]);
  int64_t e = before1 + before2 + (i - s * b);
  if (kg == 1) e += min((s + 1) * p.b[0], p.n[0]) - before1;
  p.pos_h[e] = h; p.pos_r[e] = r; p.pos_t[e] = t;
}

}  // namespace mke

extern "C" int mke_epoch_positives(const int32_t* list1, const int32_t* list2, int64_t n1, int64_t n2, const int64_t* perm1,
                                   const int64_t* perm2, int64_t b1, int64_t b2, int64_t n_steps, int32_t* list1_out,
                                   int32_t* list2_out, int32_t* pos_h, int32_t* pos_r, int32_t* pos_t, void* stream) {
  using namespace mke;
  if (n1 < 0 || n2 < 0 || b1 < 0 || b2 < 0 || n_steps < 0) { set_error("mke_epoch_positives: negative count"); return MKE_E_SHAPE; }
  if (n1 + n2 > 0x7FFFFFFFLL) { set_error("mke_epoch_positives: more than 2^31 - 1 positives"); return MKE_E_SHAPE; }
  if (n1 + n2 == 0) return MKE_OK;
  if ((n1 && !list1) || (n2 && !list2) || !pos_h || !pos_r || !pos_t) { set_error("mke_epoch_positives: NULL pointer"); return MKE_E_NULL; }
  if ((list1_out && list1_out == list1) || (list2_out && list2_out == list2)) { set_error("mke_epoch_positives: a list cannot be shuffled in place"); return MKE_E_SHAPE; }
  EpochParams p;
  p.list_in[0] = list1; p.list_in[1] = list2; p.list_out[0] = list1_out; p.list_out[1] = list2_out;
  p.perm[0] = perm1; p.perm[1] = perm2; p.n[0] = n1; p.n[1] = n2; p.b[0] = b1; p.b[1] = b2; p.n_steps = n_steps;
  p.pos_h = pos_h; p.pos_r = pos_r; p.pos_t = pos_t;
  const int64_t blocks = (n1 + n2 + MKE_BLOCK - 1) / MKE_BLOCK;
  hipLaunchKernelGGL(k_epoch_positives, dim3((unsigned)blocks), dim3(MKE_BLOCK), 0, (hipStream_t)stream, p);
  return check_launch("k_epoch_positives");
}
