// C ABI (include/camo_fusion.h): the launch schedules of the fused forward / backward of the fusion
// model, over the workspace that fusion_ws.h lays out.  No device code here.
//
// Algebra used (results equal to the reference up to fp32 re-association):
//   * mean-pool linearity.  The reference computes Z = Y + FFN(Y) for every node and then only
//     uses mean_t Z (fusion_model.py:120,134).  Since the second FFN layer is linear,
//       mean_t Z = mean_t Y + (mean_t H1d) . W2^T + b2,   H1d = dropout(relu(Y.W1^T + b1)),
//     so the [Nr,512]x[512,256] GEMM per sample (22 % of the forward FLOPs) becomes a
//     [B,512]x[512,256] one, and in the backward d(H1d) is one row per sample broadcast
//     through the ReLU/dropout mask, dW2 = d(pool)^T . mean(H1d)  (two more full-size GEMMs gone).
//   * K|V projections share their input, so they run as one N=2H GEMM on the contiguous rows
//     H..3H of in_proj_weight; their input gradients as one K=2H GEMM.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/camo_fusion.h"

#include "attn.h"
#include "gemm.h"
#include "fused_rows.h"
#include "tail_wide.h"
#include "attn_maps.h"
#include "gemm16.h"
#include "misc.h"
#include "abi_util.h"
#include "fusion_ws.h"

namespace {
thread_local std::string g_err;
}  // namespace

// the error return of every ABI file (abi_util.h), defined next to the string it sets
int camo_abi::fail(int code, const std::string& msg) { g_err = msg; return code; }
int camo_abi::fail_hip(int e, const char* where) {
  g_err = std::string(where) + ": " + hipGetErrorString((hipError_t)e);
  return CAMO_E_HIP;
}
using namespace camo_abi;
using namespace camo_ws;

namespace {

// Schedule options are the CALLER's (camo_options_t behind camo_dims_t::options); these are the defaults (options == NULL)
constexpr camo_options_t k_default_options = {/*sched16*/ -1, /*fused*/ -1, /*tail17*/ -1, /*fused_rt*/ -1, /*wide2*/ -1, /*fused_one*/ 1, /*wide_front_rt*/ 0,
                                              /*tailw*/ -1, /*tailw_bwd*/ -1, /*param_space*/ -1, /*tn_big*/ -1, /*fused_variant*/ 1, /*back_lead*/ 1,
                                              /*tn_balance*/ 1, /*tn_kcap*/ 0, /*tn_exp*/ 0, /*exp*/ 0, /*fused_save*/ 0, /*tail_skip_arrival*/ 0, /*wide2_bwd*/ -1};
unsigned long long* g_dbg_stamps = nullptr;   // developer timeline buffer of the fused kernels (camo_debug_set_stamps; like camo_prof_*: a profiling facility, not a schedule option)
int g_dbg_stamp_blocks = 0;


// The hand-offs of one entry-point call: state that one launch sequence leaves for a later one of the same call.  Built on the entry
// point's stack and passed down by reference.  No option or per-call state lives in the library, so two engines in one process (or two
// threads) cannot change each other's schedule or hand-offs.  (Decisions are not hand-offs: they are in the plan.)
struct Call {
  // camo_forward_cached / camo_forward_loss_backward: caller-owned weight shadows (camo_shadow_bytes), null otherwise.  The 14
  // fragment-order bf16 copies the fused kernels stream live there instead of in the per-batch workspace, so that the optimizer call
  // can leave them ready for the next step (camo_clip_adamw_shadows) and the forward need not rebuild them (shadows_valid).
  void* shadows = nullptr;
  bool shadows_valid = false;
  bool fold_missing = false;          // camo_forward_cached(shadows_valid = 2): valid shadows that lack the inference calls' folded in-projection
  int shadows_state = 0;              // what the fused forward left in them: 0 untouched, 1 forward set, 2 forward + transposed
  // clears that a forward without a shadow launch leaves to the first backward kernel (forward_nodes17 -> backward_nodes17)
  void* zero_bwd1_ptr[FUSED_BWD1_MAXZ]; unsigned zero_bwd1_bytes[FUSED_BWD1_MAXZ]; int nzero_bwd1 = 0;
  hipEvent_t tail_event = nullptr;    // camo_forward_loss_backward's optional event (record_tail_event)
  int tail_skip = 0;                  // the caller's one-shot tail_skip_arrival: read by the entry points that can launch the one-launch tail,
  bool tail_skip_taken = false;       // which write 0 back to the caller's options once that launch took it
};
const camo_options_t& options_of(const camo_dims_t* d) { return *(d && d->options ? d->options : &k_default_options); }

typedef unsigned short us;

int check_dims(const camo_dims_t* d, int B, int T, int Nk) {
  if (!d) return fail(CAMO_E_ARG, "dims is null");
  if (B < 1 || T < B || Nk < 1) return fail(CAMO_E_ARG, "need B >= 1, T >= B (every sample has >= 1 RG row), Nk >= 1");
  if (d->rg_dim < 1 || d->kg_dim < 1 || d->hidden_dim < 4 || d->num_classes < 1 || d->num_classes > 64)
    return fail(CAMO_E_ARG, "bad model dimensions");
  if (!(d->dropout >= 0.f && d->dropout < 1.f)) return fail(CAMO_E_ARG, "dropout must be in [0,1)");
  if (d->fusion_type == CAMO_FUSION_CROSS_ATTENTION) {
    if (d->num_heads < 1 || d->hidden_dim % d->num_heads) return fail(CAMO_E_ARG, "hidden_dim must be divisible by num_heads");
    if (d->hidden_dim % 2) return fail(CAMO_E_UNSUPPORTED, "hidden_dim must be even");
    if (!attn_supported(d->hidden_dim, d->num_heads, Nk))
      return fail(CAMO_E_UNSUPPORTED, "attention kernels support num_heads <= 256, head_dim <= 256, Nk <= 64 within 160 KB of LDS");
    if (!ln_supported(d->hidden_dim)) return fail(CAMO_E_UNSUPPORTED, "LayerNorm kernels support hidden_dim <= 1024");
  } else if (d->fusion_type == CAMO_FUSION_LATE) {
    if (d->hidden_dim % 4) return fail(CAMO_E_UNSUPPORTED, "late fusion needs hidden_dim divisible by 4");
  } else {
    return fail(CAMO_E_ARG, "unknown fusion_type");
  }
  if ((double)T * d->hidden_dim * 2 > 2.0e9 || (double)T * d->num_heads * Nk > 4.0e9)
    return fail(CAMO_E_UNSUPPORTED, "batch too large for 32-bit element indices");
  return 0;
}

void set_res(GemmProb& p, const float* res, int ldr) { p.res = res; p.ldr = ldr; }
void set_drop(GemmProb& p, uint32_t site) { p.flags |= GF_DROPOUT; p.drop_site = site; }
void set_bcast(GemmProb& p, const float* v, int ldv, const int* row_sample, const float* inv_nr, int uniform_n) {
  p.flags |= GF_RES_BCAST; p.res = v; p.ldr = ldv; p.row_sample = row_sample; p.inv_nr = inv_nr; p.uniform_n = uniform_n;
}

// ---- the bf16 schedule's GEMM batch (gemm16.h) ------------------------------------------------
struct GB16 {
  Gemm16Batch b; Gemm16Knobs kn; hipStream_t st;
  GB16(const DropCfg& d, const camo_options_t& o, hipStream_t st_) : st(st_) {
    std::memset(&b, 0, sizeof(b)); b.drop = d;
    kn.tn_big = o.tn_big; kn.balance = o.tn_balance; kn.tn_kcap = o.tn_kcap; kn.exp = o.tn_exp;
  }
  Gemm16Prob& add() { Gemm16Prob& p = b.p[b.n++]; std::memset(&p, 0, sizeof(p)); p.aux_scale = 1.f; return p; }
  // y = x.W^T (+bias): x16 [M,K], W16 [N,K]; fp32 result y and/or bf16 result y16 (either may be null)
  Gemm16Prob& nt(const us* x, int ldx, const us* W, int ldw, const float* bias, float* y, int ldy, us* y16, int ldy16,
                 int M, int N, int K, int flags = 0) {
    Gemm16Prob& p = add();
    p.A = x; p.lda = ldx; p.B = W; p.ldb = ldw; p.bias = bias; p.C = y; p.ldc = ldy; p.C16 = y16; p.ldc16 = ldy16;
    p.M = M; p.N = N; p.K = K; p.flags = flags;
    return p;
  }
  // dW [Nout, Nin] += dy^T.x : dy16 [rows, Nout], x16 [rows, Nin]; db [Nout] += colsum(dy)
  Gemm16Prob& tn(const us* dy, int lddy, const us* x, int ldx, float* dW, int lddw, float* db, int Nout, int Nin, int rows) {
    Gemm16Prob& p = add();
    p.A = dy; p.lda = lddy; p.B = x; p.ldb = ldx; p.C = dW; p.ldc = lddw; p.bias_grad = db;
    p.M = Nout; p.N = Nin; p.K = rows; p.flags = GF_A_KMAJOR | GF_B_KMAJOR | GF_ATOMIC;
    return p;
  }
  int run() {
    if (b.n == 0) return 0;
    int e = launch_gemm16_batch(b, kn, st);
    b.n = 0;
    return e;
  }
};
void set_res(Gemm16Prob& p, const float* res, int ldr) { p.res = res; p.ldr = ldr; }
void set_drop(Gemm16Prob& p, uint32_t site) { p.flags |= GF_DROPOUT; p.drop_site = site; }
void set_bcast(Gemm16Prob& p, const float* v, int ldv, const int* row_sample, const float* inv_nr, int uniform_n) {
  p.flags |= GF_RES_BCAST; p.res = v; p.ldr = ldv; p.row_sample = row_sample; p.inv_nr = inv_nr; p.uniform_n = uniform_n;
}

// ---- the launch schedule of one call ----------------------------------------------------------------------
// Which kernels a call runs follows from its arguments.  make_plan() is the one place that rule lives: a pure
// function of the caller's options, the dims and the call's arguments (PlanIn), evaluated once per entry-point call; everything
// below it takes its decisions from the camo_plan_t it returns (include/camo_fusion.h documents the fields; camo_debug_plan shows
// it to the tests, tests/test_schedule_plan.py pins the table).
enum CallKind { CALL_INFERENCE, CALL_FORWARD_SAVE /* a camo_backward follows */, CALL_BACKWARD, CALL_TRAIN /* camo_forward_loss_backward: labels ride along */ };
struct PlanIn {
  const camo_options_t& o; const camo_dims_t& d;
  bool rg_proj, kg_proj;        // the projection weights are present
  int precision, B, T, Nk, max_nr;
  CallKind kind;
  bool attn_maps;               // attention maps are wanted: pointers given, or CAMO_FLAG_ATTN_MAPS
  bool fused_maps;              // CAMO_FWD_FUSED_MAPS: an inference call that wants maps may take the fused schedule + the maps launch
  int cus;                      // compute units of the device (the one-launch tail's blocks must be co-resident)
};

// the fused row-tile kernels' forward launches (fused_rows.h) of a call that takes that schedule
static void plan_fused_forward(const PlanIn& in, bool save, bool param_space, camo_plan_t& p) {
  const camo_options_t& o = in.o;
  const int B = in.B, T = in.T, max_nr = in.max_nr, C = in.d.num_classes;
  const bool infer = in.kind == CALL_INFERENCE, train = in.kind == CALL_TRAIN;
  // Which tile family the two halves take: 0 = 32-row tiles, one per block of 4 waves (small batches: one tile per CU is all there
  // is); 2 / 4 = that many tiles per block of 8 waves (fused_wide.hip), chosen so that the blocks still fill the chip.
  int rt = o.fused_rt;
  // by size: inference calls from about half a 128-row block per CU on (64-row blocks below that).  Calls that save for a backward stay on the 32-row kernels:
  // the saved-tensor stores of the one-launch kernel are not tuned yet (measured slower: B = 64 step 0.53 vs 0.40 ms)
  // (measured eval forward, us: B = 32 [13.5 k rows] 87 / 85 / 103 for 32-row / 2 / 4 tiles per block; B = 48 [20 k] 116 / 103 / 106; B = 56 [24 k] 131 / 112 / 108)
  if (rt < 0) rt = save ? 0 : (T >= 22528 ? 4 : (T >= 13312 ? 2 : 0));
  if (rt != 0 && rt != 1 && rt != 2 && rt != 4) rt = 0;
  if (rt && max_nr > wide_max_rows(rt) - 64 * rt) rt = 0;
  // A call that produces its maps behind the forward (p.maps, csrc/attn_maps.hip) needs q, k2 | v2 in the workspace: the one-launch
  // kernels of the RG rows keep them in registers, so it takes the two-launch combinations the saving forwards run -- the 32-row
  // front half below 10 240 packed rows, the wide front half from there on, and the 32-row back half (the one that stores lse2).
  const bool maps = p.maps != 0;
  if (maps) rt = 0;
  // The RG rows' whole forward in one launch of 64-row half-blocks, two independent blocks per CU, + the KG rows' launch behind it
  // (fused_wide2.hip).  By size for inference AND training calls (the saving / dropout variants write the backward's saved set); a
  // forced fused_rt selects the 8-wave / 32-row kernels.
  bool rg64 = !maps && o.wide2 != 0 && o.fused_one != 0 && max_nr <= wide2_max_rows();
  // training calls from 57 344 rows: their blocks are twice as long (the saved set, the dropout hashes), so the second round of blocks
  // must be nearly full before they beat the 32-row back half (measured, ms per step without / with: B = 96 0.517 / 0.540, B = 128
  // 0.637 / 0.621, B = 192 0.864 / 0.804, B = 256 1.076 / 0.979)
  // inference calls from 10 240 rows (eval forward, us without / with: B = 16 59 / 66, B = 24 72.5 / 69.8, B = 32 77 / 71, B = 48 101 / 82)
  if (rg64 && o.wide2 < 0) rg64 = o.fused_rt < 0 && o.wide_front_rt == 0 && T >= (save ? 57344 : 10240);
  // the RG rows in one launch: the 64-row kernel, or the wide tiles' (rt >= 2)
  const bool rg_one = rg64 || (rt >= 2 && o.fused_one != 0);
  // Training calls (save): the front half alone on wide blocks -- 64-row blocks from 10 240 packed rows (front 21 -> 17 us at B = 24,
  // 31 -> 26 at B = 48, 37 -> 28 at B = 56), 128-row blocks from 28 672.  -> sub-tiles per block, 0 = the 32-row front kernel.
  // (the back half of training calls stays on the 32-row kernel, whose saving + dropout variant is the faster one: 77 vs 94 us at B = 64)
  const bool rows128 = T >= 4 * 32 * 224;
  int wf_rt = 0;
  if ((save || maps) && rt == 0 && o.fused_rt < 0 && o.wide_front_rt >= 0 && (T >= 10240 || o.wide_front_rt > 0)) {
    wf_rt = o.wide_front_rt > 0 ? o.wide_front_rt : (rows128 ? 4 : 2);
    if ((wf_rt != 1 && wf_rt != 2 && wf_rt != 4) || max_nr > wide_max_rows(wf_rt) - 64 * wf_rt) wf_rt = 0;
  }
  p.save = save;
  if (rg_one) p.front = CAMO_FRONT_KG;
  else if (rt || wf_rt) { p.front = CAMO_FRONT_WIDE; p.front_rt = rt ? rt : wf_rt; }
  else p.front = CAMO_FRONT_ROWS32;
  if (rg64) {
    p.back = CAMO_BACK_RG_64;
    // (R16 is read by the row-space form of the projections' weight gradients only; tests that read it back run an inference call with fused_save)
    p.save_r16 = !param_space || o.fused_save != 0;
  } else if (rt) { p.back = rg_one ? CAMO_BACK_RG_WIDE : CAMO_BACK_WIDE; p.back_rt = rt; }
  else p.back = CAMO_BACK_ROWS32;

  // The per-sample tail.  The two-plane launch's weight planes are built by extra blocks of a wide front launch (CAMO_FRONT_KG or
  // CAMO_FRONT_WIDE), so both two-plane rules below are written on top of the front launch's.
  const bool one_launch = o.tail17 != 0 && tail_fused_ok(B, C, in.cus);
  // inference calls behind the RG rows' one-launch forward
  // (B <= 32: the grouped fp32 tail, forward only, is the shorter one: 29.8 vs 33.5 us at B = 32; equal at 48)
  const bool planes_infer = infer && o.tailw != 0 && rg_one && tail_wide_ok(B, C) && (o.tailw > 0 || B > 32 || !tail_fused_ok(B, C, in.cus));
  // training calls from the 128-row front half's size on (wf_rt: also behind the RG rows' one-launch forward) with more than 64 samples: the tail's FORWARD as the one two-plane launch (with fp32
  // copies of what the backward launches read) instead of four fp32 GEMM launches (B = 256: 4 x 27 us -> 34 us); the loss launch
  // (heads_loss_kernel) and the backward follow -- the backward as ONE two-plane launch for the tail's input-gradient chain + ONE
  // launch for its weight gradients, instead of four fp32 GEMM launches that each pair an input gradient with a weight gradient
  // (B = 256: 108 us), unless tailw_bwd = 0
  const bool planes_train = train && heads_loss_ok(B, C) && B > 64 && o.tailw != 0 && rows128 && wf_rt != 0 && tail_wide_ok(B, C);
  if (planes_infer) p.tail = CAMO_TAIL_PLANES;
  else if ((infer || train) && one_launch) p.tail = CAMO_TAIL_ONE_LAUNCH;
  else if (planes_train) p.tail = o.tailw_bwd != 0 ? CAMO_TAIL_PLANES_TRAIN : CAMO_TAIL_PLANES_TRAIN_FWD;
  else p.tail = CAMO_TAIL_GEMMS;
  if (train && p.tail == CAMO_TAIL_ONE_LAUNCH) {
    p.loss = CAMO_LOSS_TAIL;
    // The kernel leaves copies of the operands of its eight big weight gradients, and these gradients to a launch behind it.  One
    // group of 16 samples: extra blocks at the end of the node-level backward's first launch, which always follows, run them on CUs
    // that its row tiles leave idle (a launch of their own would cost ~5 us of floor).  More groups: the gradients are sums over
    // every group -- one batched launch (contraction over the B samples).
    p.tail_wg = B > 16 ? CAMO_TAIL_WG_LAUNCH : CAMO_TAIL_WG_BWD1;
    // the tail event: behind the launch that finishes the tail's weight gradients
    p.tail_event = p.tail_wg == CAMO_TAIL_WG_BWD1 ? CAMO_EVENT_AFTER_BWD1 : CAMO_EVENT_BEFORE_NODES;
  }
}

// the fused row-tile kernels' backward launches
static void plan_fused_backward(const PlanIn& in, bool param_space, camo_plan_t& p) {
  const camo_options_t& o = in.o;
  p.param_space = param_space;
  // the RG rows of the first half on 64-row half-blocks (bwd_wide2.hip) from 16 384 packed rows (training step, ms without / with:
  // B = 24 0.209 / 0.217, B = 32 0.2395 / 0.237, B = 48 0.307 / 0.301, B = 64 0.355 / 0.349, B = 128 0.632 / 0.615, B = 256 1.007 / 0.944,
  // B = 1024 3.215 / 2.815) -- behind either forward: the saved set is the same
  const bool bwd1w = o.wide2_bwd != 0 && (o.wide2_bwd > 0 || (o.fused_rt < 0 && in.T >= 16384));
  p.bwd1 = bwd1w ? CAMO_BWD1_64 : CAMO_BWD1_ROWS32;
  // the second half without an arrival protocol (the KG rows' dQ2 sums become bf16 in a second, B-block launch): parameter-space
  // form only, by the size rule of the wide first half: the extra launch costs ~2 us
  // (wide2_bwd == 2: developer A/B, bwd2p_kernel + bwd2_finish_kernel behind the wide first half)
  p.bwd2 = !(param_space && bwd1w) ? CAMO_BWD2_ROWS32 : (o.wide2_bwd != 2 ? CAMO_BWD2_64 : CAMO_BWD2_ROWS32_SPLIT);
}

camo_plan_t make_plan(const PlanIn& in) {
  const camo_options_t& o = in.o; const camo_dims_t& d = in.d;
  const int B = in.B, T = in.T, Nk = in.Nk, max_nr = in.max_nr;
  const bool train = in.kind == CALL_TRAIN;
  camo_plan_t p; std::memset(&p, 0, sizeof(p));
  // the training call's loss, unless the one-launch tail takes it: the head output layer, the loss and the head output layer's backward
  // as one kernel (misc.hip, heads_loss_kernel); large batches / many classes: the three steps as separate launches
  if (train) p.loss = heads_loss_ok(B, d.num_classes) ? CAMO_LOSS_HEADS : CAMO_LOSS_LAUNCH;
  if (d.fusion_type == CAMO_FUSION_LATE) {
    p.nodes = CAMO_NODES_LATE;
    if (train) p.tail_event = CAMO_EVENT_END;      // (a schedule without an earlier point)
    return p;
  }
  if (train) p.tail_event = CAMO_EVENT_BEFORE_NODES;
  const bool proj = in.rg_proj && in.kg_proj, bf16 = in.precision == CAMO_PREC_BF16;
  // calls at the reference configuration that do not ask for attention maps take the fused row-tile schedule -- and inference calls
  // that ask for them and allow it (CAMO_FWD_FUSED_MAPS): the maps then come out of one launch behind the back half
  const bool maps = in.attn_maps && in.fused_maps && in.kind == CALL_INFERENCE;
  if ((!in.attn_maps || maps) && o.fused != 0 && bf16 && fused17_dims(d) && Nk <= 16 && max_nr <= 64 * FUSED_MAX_SPLITS && proj) {
    p.nodes = CAMO_NODES_FUSED;
    p.maps = maps;
    p.shadows = in.kind != CALL_BACKWARD;      // (camo_backward takes no shadow argument)
    // The projections' and in-projections' weight gradients in parameter space (no dR / dG product in the second backward kernel, 131 k
    // instead of 427 k MACs per row, one small launch behind the weight gradients): from ~10 k packed rows on -- below that the extra launch
    // (~10 us) costs what the second kernel saves (measured: B = 16 +10 us, B = 64 -22 us, B = 256 -105 us per step).  The forward reads it
    // too: R16 is an operand of the row-space form only.
    const bool param_space = o.param_space < 0 ? T >= 10240 : o.param_space > 0;
    if (in.kind != CALL_BACKWARD) plan_fused_forward(in, in.kind != CALL_INFERENCE || o.fused_save != 0, param_space, p);
    if (in.kind == CALL_BACKWARD || train) plan_fused_backward(in, param_space, p);
    return p;
  }
  // The bf16 schedule runs when the operands can live in HBM as bf16 tiles the gemm16 kernel takes whole:
  // cross-attention fusion with both input projections, every width a multiple of 64, head_dim 32 attention
  // on the MFMA kernels.  Anything else (and option sched16 = 0) takes the general fp32-operand schedule.
  const bool use16 = o.sched16 != 0 && bf16 && proj && !(d.hidden_dim % 64) && !(d.rg_dim % 64) && !(d.kg_dim % 64) &&
                     attn_mfma_ok(d.hidden_dim, d.num_heads, Nk, max_nr, false) && attn_mfma_ok(d.hidden_dim, d.num_heads, Nk, max_nr, true) &&
                     ((double)T + 128.0) * 3.0 * d.hidden_dim * 2.0 < 4.0e9;
  p.nodes = use16 ? CAMO_NODES_BF16 : CAMO_NODES_GENERAL;
  return p;
}

// What every function below an entry point needs: the call's arguments, and -- filled by open_batch() once they are validated -- the
// caller's options, the plan, the carved descriptor and workspace (external shadows bound) and the dropout configuration.
struct Batch {
  const camo_dims_t* dims; const float* const* P; float* const* Gr; const float* rg; const int32_t* rg_offsets; const void* desc; const float* kg;
  int B, T, Nk, max_nr; void* workspace; size_t workspace_bytes; int training; uint64_t seed; int precision; hipStream_t st;
  const camo_options_t* opt; camo_plan_t plan; Desc bd; Ws w; DropCfg drop;
};

// the plan of an entry point's call (behind check_dims; params == null: left empty, open_batch refuses the call)
void plan_batch(Batch& x, CallKind kind, bool attn_maps, bool fused_maps = false) {
  x.opt = &options_of(x.dims);
  if (x.P) x.plan = make_plan(PlanIn{*x.opt, *x.dims, x.P[CAMO_P_RG_PROJ_W] != nullptr, x.P[CAMO_P_KG_PROJ_W] != nullptr, x.precision, x.B, x.T, x.Nk, x.max_nr,
                                     kind, attn_maps, fused_maps, device_cus()});
}

// (validated arguments -> the rest of the bundle; `ptrs_ok`: the entry point's own pointer arguments are there)
int open_batch(Batch& x, const Call& c, bool ptrs_ok) {
  if (!x.P || !x.rg || !x.rg_offsets || !x.desc || !x.kg || !x.workspace || !ptrs_ok) return fail(CAMO_E_ARG, "null pointer argument");
  x.bd = desc_carve(x.B, x.T, const_cast<void*>(x.desc));
  if (x.max_nr < 1 || x.max_nr > x.T) return fail(CAMO_E_ARG, "max_nr out of range");
  if (x.precision != CAMO_PREC_F32 && x.precision != CAMO_PREC_BF16) return fail(CAMO_E_ARG, "unknown precision");
  x.w = carve(*x.dims, x.B, x.T, x.Nk, x.workspace);
  if (c.shadows) x.w.f.sh = shadow_carve(c.shadows);      // (a call that was handed external shadows keeps the fused schedule's weight shadows there)
  if (x.workspace_bytes < x.w.bytes) return fail(CAMO_E_WORKSPACE, "workspace smaller than camo_workspace_bytes()");
  x.drop = make_drop(x.training, x.dims->dropout, x.seed);
  return 0;
}

// ---- the four heads (fusion_model.py:208-235), shared by both fusion types -------------------
// The per-sample ("tail") GEMMs have M = B rows and a negligible FLOP share, so they always run
// on the exact f32 MFMA; `precision` selects the MFMA type of the node-level (T-row) GEMMs only.
// labels + outputs of the native training call: where the plan puts the loss (camo_plan_t::loss)
struct FusedLoss { const int64_t* y; const float* e; const float* s; float* terms; int32_t* pred; };
GB tail_gemms(const Batch& x) { return GB(x.drop, CAMO_PREC_F32, x.st); }     // per-sample (B-row) GEMMs

// fl given: the head output layer, the loss and the head output layer's backward run as one kernel (misc.hip, heads_loss_kernel)
// instead of three launches
int heads_forward(const Batch& x, int head0, int F, float* outs, const FusedLoss* fl, bool hidden_done = false, bool defer_out_grads = false) {
  const camo_dims_t& d = *x.dims; const Ws& w = x.w;
  const float* const* hp = x.P + head0;
  const int B = x.B, Fh = F / 2, C = d.num_classes, Wd = 2 * C + 2;
  const int nout[4] = {C, C, 1, 1}, coff[4] = {0, C, 2 * C, 2 * C + 1};
  GB g = tail_gemms(x);
  if (!hidden_done) {                      // (else w.hid came out of the two-plane tail launch)
    for (int h = 0; h < 4; ++h) {
      GemmProb& p = g.nt(w.fused, F, hp[4 * h], F, hp[4 * h + 1], w.hid + h * Fh, 4 * Fh, B, Fh, F, GF_RELU);
      set_drop(p, SITE_HEAD0 + h);
    }
    CK(g.run(), "heads hidden");
  }
  if (fl) {
    float* const* hg = x.Gr + head0;
    HeadsOut ho;
    for (int h = 0; h < 4; ++h) { ho.W[h] = hp[4 * h + 2]; ho.b[h] = hp[4 * h + 3]; ho.gW[h] = hg[4 * h + 2]; ho.gb[h] = hg[4 * h + 3]; }
    CK(launch_heads_loss(w.hid, ho, reinterpret_cast<const long long*>(fl->y), fl->e, fl->s, B, C, Fh, x.drop.scale, outs, fl->terms,
                         fl->pred, w.dhid, x.st, defer_out_grads ? w.dlog : nullptr), "heads out + loss + heads out bwd");
    return 0;
  }
  for (int h = 0; h < 4; ++h)
    g.nt(w.hid + h * Fh, 4 * Fh, hp[4 * h + 2], Fh, hp[4 * h + 3], outs + coff[h], Wd, B, nout[h], Fh, h == 3 ? GF_SIGMOID : 0);
  CK(g.run(), "heads out");
  return 0;
}

// d_outs -> dfused (w.dfused, zeroed by the forward) and the 16 head-parameter gradients
int heads_backward(const Batch& x, int head0, int F, const float* outs, const float* d_outs, int pre_activation, bool heads_out_done) {
  const camo_dims_t& d = *x.dims; const Ws& w = x.w;
  const float* const* hp = x.P + head0; float* const* hg = x.Gr + head0;
  const int B = x.B, Fh = F / 2, C = d.num_classes, Wd = 2 * C + 2;
  const int nout[4] = {C, C, 1, 1}, coff[4] = {0, C, 2 * C, 2 * C + 1};
  GB g = tail_gemms(x);
  // (w.dfused was zeroed by the forward's memset of the workspace's zero block)
  if (!heads_out_done) {      // else w.dhid and the output-layer gradients came out of heads_loss_kernel
    const float* dlog = d_outs;
    if (!pre_activation) { CK(launch_head_out_grad(outs, d_outs, w.dlog, B, Wd, x.st), "head_out_grad"); dlog = w.dlog; }
    for (int h = 0; h < 4; ++h) {
      GemmProb& p = g.nn(dlog + coff[h], Wd, hp[4 * h + 2], Fh, w.dhid + h * Fh, 4 * Fh, B, Fh, nout[h]);
      set_relu_bwd(p, w.hid + h * Fh, 4 * Fh, x.drop.scale);
      g.tn(dlog + coff[h], Wd, w.hid + h * Fh, 4 * Fh, hg[4 * h + 2], Fh, hg[4 * h + 3], nout[h], Fh, B);
    }
    CK(g.run(), "heads out bwd");
  }
  for (int h = 0; h < 4; ++h) {
    g.nn(w.dhid + h * Fh, 4 * Fh, hp[4 * h], F, w.dfused, F, B, F, Fh, GF_ATOMIC);
    g.tn(w.dhid + h * Fh, 4 * Fh, w.fused, F, hg[4 * h], F, hg[4 * h + 1], Fh, F, B);
  }
  CK(g.run(), "heads hidden bwd");
  return 0;
}

// The eight big weight gradients of the cross-attention tail, dW [rows][cols] += dy^T x over the B samples (db += colsum(dy)): the
// heads' hidden layers, fusion layers 3 and 0, the pooled FFN layers.  f(dy, ld_dy, x, ld_x, dW, db, rows, cols), in the order every
// launch that sums them keeps (fp32 sums, some with atomics: the order is part of the result).
template <typename F> void for_tail_wg(const Batch& b, F&& f) {
  const Ws& w = b.w; float* const* Gr = b.Gr;
  const int H = b.dims->hidden_dim, Fh = H / 2;
  for (int h = 0; h < 4; ++h) f(w.dhid + h * Fh, 4 * Fh, w.fused, H, Gr[CAMO_P_HEADS + 4 * h], Gr[CAMO_P_HEADS + 4 * h + 1], Fh, H);
  f(w.dfused, H, w.F1, H, Gr[CAMO_P_FU_W3], Gr[CAMO_P_FU_B3], H, H);
  f(w.dF1, H, w.comb, 2 * H, Gr[CAMO_P_FU_W0], Gr[CAMO_P_FU_B0], H, 2 * H);
  f(w.dcomb, 2 * H, w.H1mean, 2 * H, Gr[CAMO_P_F1_W3], Gr[CAMO_P_F1_B3], H, 2 * H);
  f(w.dcomb + H, 2 * H, w.H2mean, 2 * H, Gr[CAMO_P_F2_W3], Gr[CAMO_P_F2_B3], H, 2 * H);
}
void add_tail_wg(const Batch& b, GB& g) {
  for_tail_wg(b, [&](const float* dy, int ld_dy, const float* x, int ld_x, float* dW, float* db, int rows, int cols) { g.tn(dy, ld_dy, x, ld_x, dW, cols, db, rows, cols, b.B); });
}

// ---- node-level forward of the bf16 schedule: CrossAttentionFusion.forward, fusion_model.py:75-135 ----
int forward_nodes16(const Batch& x, float* attn_rg2kg, float* attn_kg2rg) {
  const camo_dims_t& d = *x.dims; const float* const* P = x.P; const Ws& w = x.w; const DropCfg& drop = x.drop; hipStream_t st = x.st;
  const float* rg = x.rg; const float* kg = x.kg; const int32_t* rg_offsets = x.rg_offsets;
  const int32_t* row_sample = x.bd.row_sample; const float* inv_nr = x.bd.inv_nr;
  const int B = x.B, T = x.T, Nk = x.Nk, max_nr = x.max_nr;
  const int H = d.hidden_dim, D = d.rg_dim, Dk = d.kg_dim, TK = B * Nk, nh = d.num_heads;
  const size_t HH = (size_t)H * H;
  const Ws::H16& h = w.h;
  {   // prep: clear the atomics block and the pad rows, cast the inputs and the node-level weights to bf16
    PrepBatch pb; pb.n = 0;
    auto job = [&](int type, const float* src, void* dst, size_t n, int rows, int cols, int ld, int off) {
      PrepJob& J = pb.j[pb.n++];
      J.type = type; J.src = src; J.dst = dst; J.n = n; J.rows = rows; J.cols = cols; J.ld_dst = ld; J.col_off = off; J.blk_begin = 0;
    };
    auto cast = [&](const float* src, us* dst, size_t n) { job(PREP_CAST, src, dst, n, 0, 0, 0, 0); };
    auto castT = [&](const float* src, us* dst, int rows, int cols, int ld, int off) { job(PREP_CAST_T, src, dst, 0, rows, cols, ld, off); };
    // the atomics block: pooled means and dfused (this schedule accumulates nothing into dKV)
    job(PREP_ZERO, nullptr, w.zero_base, w.zero_fwd_bytes, 0, 0, 0, 0);
    cast(rg, h.X, (size_t)T * D); cast(kg, h.KG, (size_t)TK * Dk);
    cast(P[CAMO_P_RG_PROJ_W], h.Wrg, (size_t)H * D); cast(P[CAMO_P_KG_PROJ_W], h.Wkg, (size_t)H * Dk);
    cast(P[CAMO_P_A1_IN_W], h.Win1, 3 * HH); cast(P[CAMO_P_A2_IN_W], h.Win2, 3 * HH);
    cast(P[CAMO_P_A1_OUT_W], h.Wo1, HH); cast(P[CAMO_P_A2_OUT_W], h.Wo2, HH);
    cast(P[CAMO_P_F1_W0], h.W1, 2 * HH); cast(P[CAMO_P_F2_W0], h.W2, 2 * HH);
    castT(P[CAMO_P_F1_W0], h.W1T, 2 * H, H, 2 * H, 0); castT(P[CAMO_P_F2_W0], h.W2T, 2 * H, H, 2 * H, 0);
    castT(P[CAMO_P_A1_OUT_W], h.Wo1T, H, H, H, 0); castT(P[CAMO_P_A2_OUT_W], h.Wo2T, H, H, H, 0);
    castT(P[CAMO_P_A1_IN_W], h.WcRgT, H, H, 3 * H, 0); castT(P[CAMO_P_A2_IN_W] + HH, h.WcRgT, 2 * H, H, 3 * H, H);
    castT(P[CAMO_P_A2_IN_W], h.WcKgT, H, H, 3 * H, 0); castT(P[CAMO_P_A1_IN_W] + HH, h.WcKgT, 2 * H, H, 3 * H, H);
    for (int i = 0; i < h.pad.n; ++i) job(PREP_ZERO, nullptr, h.pad.r[i].ptr, h.pad.r[i].bytes, 0, 0, 0, 0);
    CK(launch_prep(pb, st), "prep (clear + bf16 casts)");
  }
  GB16 g(drop, *x.opt, st);
  // input projections: fp32 for the residual stream, bf16 for the GEMMs that read them
  g.nt(h.KG, Dk, h.Wkg, Dk, P[CAMO_P_KG_PROJ_B], w.G, H, h.G, H, TK, H, Dk);
  g.nt(h.X, D, h.Wrg, D, P[CAMO_P_RG_PROJ_B], w.R, H, h.R, H, T, H, D);
  CK(g.run(), "input projections");
  // in-projections of both attention blocks (packed in_proj_weight: rows 0..H-1 = Wq, H..3H-1 = Wk|Wv)
  g.nt(h.R, H, h.Win1, H, P[CAMO_P_A1_IN_B], w.Q, H, nullptr, 0, T, H, H);
  g.nt(h.R, H, h.Win2 + HH, H, P[CAMO_P_A2_IN_B] + H, w.KV2, 2 * H, nullptr, 0, T, 2 * H, H);
  g.nt(h.G, H, h.Win1 + HH, H, P[CAMO_P_A1_IN_B] + H, w.KV, 2 * H, nullptr, 0, TK, 2 * H, H);
  g.nt(h.G, H, h.Win2, H, P[CAMO_P_A2_IN_B], w.Q2, H, nullptr, 0, TK, H, H);
  CK(g.run(), "attention in-projections");
  // both attention directions in one launch; their outputs are GEMM operands only, so they are written as bf16
  CK(launch_attn_fwd_pair(w.Q, w.KV, w.Q2, w.KV2, rg_offsets, w.P, w.P2, Bf16Dst{h.O, H}, Bf16Dst{h.O2, H}, w.O2, B, max_nr, H, nh, Nk,
                          drop, st), "attention fwd (both directions)");
  if (attn_rg2kg) CK(launch_attn_avg_site(w.P, attn_rg2kg, T, nh, Nk, SITE_ATTN_RG2KG, drop, st), "attn avg rg2kg");
  if (attn_kg2rg) CK(launch_attn_avg(w.P2, attn_kg2rg, T, nh, Nk, drop, st), "attn avg");
  // out-projection + residual (fusion_model.py:119,130), then LayerNorm.  At hidden_dim 256 a block of the GEMM owns
  // whole rows and the LayerNorm (with the mean pool of its output) is its epilogue.
  if (H == 256) {
    Gemm16Prob& p1 = g.nt(h.O, H, h.Wo1, H, P[CAMO_P_A1_OUT_B], w.U, H, h.Y, H, T, H, H);
    set_res(p1, w.R, H);
    p1.ln_mode = 1; p1.ln_gamma = P[CAMO_P_LN1_W]; p1.ln_beta = P[CAMO_P_LN1_B]; p1.ln_stats = w.st1;
    p1.colmean = w.Ymean; p1.ldm = H; p1.row_sample = row_sample; p1.inv_nr = inv_nr;
    Gemm16Prob& p2 = g.nt(h.O2, H, h.Wo2, H, P[CAMO_P_A2_OUT_B], w.U2, H, h.Y2, H, TK, H, H);
    set_res(p2, w.G, H);
    p2.ln_mode = 1; p2.ln_gamma = P[CAMO_P_LN2_W]; p2.ln_beta = P[CAMO_P_LN2_B]; p2.ln_stats = w.st2;
    p2.colmean = w.Y2mean; p2.ldm = H; p2.uniform_n = Nk;
    CK(g.run(), "attention out-projections + layernorm");
  } else {
    set_res(g.nt(h.O, H, h.Wo1, H, P[CAMO_P_A1_OUT_B], w.U, H, nullptr, 0, T, H, H), w.R, H);
    set_res(g.nt(h.O2, H, h.Wo2, H, P[CAMO_P_A2_OUT_B], w.U2, H, nullptr, 0, TK, H, H), w.G, H);
    CK(g.run(), "attention out-projections");
    // (the mean pools of Y and of the FFN activations are accumulated by the kernels that produce them)
    LnSeg s0{w.U, w.Y, w.st1, P[CAMO_P_LN1_W], P[CAMO_P_LN1_B], T, h.Y, w.Ymean, row_sample, inv_nr, 0};
    LnSeg s1{w.U2, w.Y2, w.st2, P[CAMO_P_LN2_W], P[CAMO_P_LN2_B], TK, h.Y2, w.Y2mean, nullptr, nullptr, Nk};
    CK(launch_ln_fwd(s0, s1, H, st), "layernorm fwd");
  }
  // FFN first layers (ReLU + dropout fused), fusion_model.py:53-65.  The activation itself is kept only as bf16 (its
  // sign pattern is the backward mask); its per-sample mean, which the pooled second layer consumes, comes out of
  // the fp32 accumulators in the epilogue.
  {
    Gemm16Prob& p1 = g.nt(h.Y, H, h.W1, H, P[CAMO_P_F1_B0], nullptr, 0, h.H1, 2 * H, T, 2 * H, H, GF_RELU);
    set_drop(p1, SITE_FFN_RG);
    p1.colmean = w.H1mean; p1.ldm = 2 * H; p1.row_sample = row_sample; p1.inv_nr = inv_nr;
    Gemm16Prob& p2 = g.nt(h.Y2, H, h.W2, H, P[CAMO_P_F2_B0], nullptr, 0, h.H2, 2 * H, TK, 2 * H, H, GF_RELU);
    set_drop(p2, SITE_FFN_KG);
    p2.colmean = w.H2mean; p2.ldm = 2 * H; p2.uniform_n = Nk;
  }
  CK(g.run(), "ffn layer 0");
  return 0;
}

// ---- node-level forward of the fused row-tile schedule: the same function in 3 launches (fused_rows.h) ----
int forward_nodes17(Call& c, const Batch& x, float* attn_rg2kg, float* attn_kg2rg) {
  const camo_plan_t& pl = x.plan; const float* const* P = x.P; const Ws& w = x.w; hipStream_t st = x.st;
  const int H = 256, B = x.B, T = x.T, Nk = x.Nk, TK = B * Nk, max_nr = x.max_nr;
  const size_t HH = (size_t)H * H;
  const bool save = pl.save != 0;
  const Ws::F17& f = w.f; const ShadowSet& sh = f.sh;
  FrontArgs fa; std::memset(&fa, 0, sizeof(fa));
  {   // weight shadows (bf16, fragment order) + the clear of the step's atomics block
    ShadowBatch sb; std::memset(&sb, 0, sizeof(sb));
    const bool build = !c.shadows_valid;        // (valid: camo_clip_adamw_shadows left them ready; only the clears ride in this launch)
    if (c.shadows) c.shadows_state = save ? 2 : 1;
    // One job per shadow, its sources the slices k_shadow_slices gives it: the shadow of [s0; s1] (N rows of K columns), or of its
    // transpose (transposed: the sources have K rows of N columns) -- the backward's dy . W products, K-concatenated where one
    // product serves three in-projections.  The jobs of a pass run in the order the shadows are carved in.
    auto jobs = [&](int transposed) {
      const int first = sb.n;
      for (const ShadowSlice& s : k_shadow_slices) {
        if (transposed && !s.trans) continue;
        us16* const dst = sh.*(transposed ? s.trans : s.plain);
        if (!sb.n || sb.j[sb.n - 1].dst != dst) {
          ShadowJob& J = sb.j[sb.n++];
          J.dst = dst; J.N = transposed ? s.cols : s.pN; J.K = transposed ? s.tK : s.cols; J.transposed = transposed;
        }
        ShadowJob& J = sb.j[sb.n - 1];
        J.src[J.nsrc] = P[s.param] + (size_t)s.r0 * s.cols; J.rows[J.nsrc] = s.rows; J.ld[J.nsrc++] = s.cols;
      }
      for (int i = first + 1; i < sb.n; ++i)
        for (int j = i; j > first && sb.j[j].dst < sb.j[j - 1].dst; --j) std::swap(sb.j[j], sb.j[j - 1]);
    };
    if (build) { jobs(0); if (save) jobs(1); }
    // The step's clears.  They ride in the shadow launch; a step without one (!build) says per range where instead: EARLY at the end of
    // the front kernel's blocks (first use: the back kernel's pooled sums), LATE in extra blocks of the first backward kernel
    // (first use: the weight-gradient launch)
    constexpr bool EARLY = true, LATE = false;
    const char* zerr = nullptr;
    auto zero = [&](void* ptr, size_t bytes, bool early) {
      bytes = (bytes + 15) & ~size_t(15);
      if (!bytes || zerr) return;
      if (build) { sb.zero_ptr[sb.nzero] = ptr; sb.zero_bytes[sb.nzero++] = bytes; }
      else if (bytes > 0xFFFFFFF0ull) zerr = "clear range too large";
      else if (early && fa.nzero >= FUSED_FRONT_MAXZ) zerr = "too many early clear ranges";
      else if (early) { fa.zero_ptr[fa.nzero] = ptr; fa.zero_bytes[fa.nzero++] = (unsigned)bytes; }
      else if (c.nzero_bwd1 >= FUSED_BWD1_MAXZ) zerr = "too many late clear ranges";
      else { c.zero_bwd1_ptr[c.nzero_bwd1] = ptr; c.zero_bwd1_bytes[c.nzero_bwd1++] = (unsigned)bytes; }
    };
    if (save) {
      zero(w.zero_base, w.zero_bytes, EARLY);                // means, dfused, arrival counters, dK|dV and dQ2 sums
      for (int i = 0; i < f.pad.n; ++i) zero(f.pad.r[i].ptr, f.pad.r[i].bytes, LATE);      // pad rows of every weight-gradient operand
      zero(w.dHm1, (size_t)B * 2 * H * sizeof(float), EARLY); zero(w.dHm2, (size_t)B * 2 * H * sizeof(float), EARLY);   // atomically summed by the one-launch tail
    } else {
      zero(w.zero_base, w.zero_fwd_bytes, EARLY);
      // (the one-launch tail's all-reduce buffers and counter words; the parameter-space block behind them belongs to the backward)
      zero(w.tailsum.F1sum, w.tailsum.bytes, EARLY);
    }
    if (zerr) return fail(CAMO_E_ARG, zerr);
    // inference calls: the RG rows' folded in-projection rides with every rebuild of the forward set, and alone when the caller's valid
    // shadows come from the optimizer call, which does not build it (camo_forward_cached, shadows_valid = 2)
    const bool fold = !save && (build || c.fold_missing);
    if (build) CK(launch_weight_shadows(sb, st), "weight shadows");
    if (fold) CK(launch_fold_rg(P[CAMO_P_A1_IN_W], P[CAMO_P_A2_IN_W] + HH, P[CAMO_P_A1_IN_B], P[CAMO_P_A2_IN_B] + H, P[CAMO_P_RG_PROJ_W], P[CAMO_P_RG_PROJ_B],
                                sh.Wf_rg, sh.bf_rg, st), "folded in-projection");
  }
  fa.qscale = 1.0f / sqrtf(32.0f); fa.save = save ? 1 : 0;
  fa.s[0] = FrontStream{x.rg, T, sh.Wrg, P[CAMO_P_RG_PROJ_B], sh.Wqkv_rg, P[CAMO_P_A1_IN_B], P[CAMO_P_A2_IN_B] + H, f.X16, f.R16, f.Q16, f.KV2_16, 0};
  fa.s[1] = FrontStream{x.kg, TK, sh.Wkg, P[CAMO_P_KG_PROJ_B], sh.Wqkv_kg, P[CAMO_P_A2_IN_B], P[CAMO_P_A1_IN_B] + H, f.KG16, f.G16, f.Q2_16, f.KV16, 0};
  fa.stamps = g_dbg_stamps; fa.exp = x.opt->exp;
  if (pl.tail >= CAMO_TAIL_PLANES) {
    // the per-sample tail's weights as hi / lo bf16 planes in fragment order: extra blocks of the (KG rows') wide front launch
    const float* hsrc[4] = {P[CAMO_P_HEADS], P[CAMO_P_HEADS + 4], P[CAMO_P_HEADS + 8], P[CAMO_P_HEADS + 12]};
    // plane of src (N rows of K columns), or of src^T (transposed: src has K rows of N columns)
    auto xj = [&](us* dst, int N, int K, int transposed, const float* src, int lo) {
      ShadowJob& J = fa.xjob[fa.nxjob++];
      std::memset(&J, 0, sizeof(J));
      J.dst = dst; J.N = N; J.K = K; J.transposed = transposed; J.nsrc = 1; J.src[0] = src; J.rows[0] = transposed ? K : N; J.ld[0] = transposed ? N : K; J.lo = lo;
    };
    // ... of the four heads' first layers [128 x 256] each, stacked: [Wh0_0; ..; Wh0_3] or its transpose (512 source rows of 256 columns)
    auto xheads = [&](us* dst, int N, int K, int transposed, int lo) {
      ShadowJob& J = fa.xjob[fa.nxjob++];
      std::memset(&J, 0, sizeof(J));
      J.dst = dst; J.N = N; J.K = K; J.transposed = transposed; J.nsrc = 4; J.lo = lo;
      for (int h = 0; h < 4; ++h) { J.src[h] = hsrc[h]; J.rows[h] = H / 2; J.ld[h] = H; }
    };
    const Ws::F17::TailPlanes& tp = f.tp;
    for (int lo = 0; lo < 2; ++lo) {
      xj(tp.W13[lo], H, 2 * H, 0, P[CAMO_P_F1_W3], lo); xj(tp.W23[lo], H, 2 * H, 0, P[CAMO_P_F2_W3], lo);
      xj(tp.Wfu0[lo], H, 2 * H, 0, P[CAMO_P_FU_W0], lo); xj(tp.Wfu3[lo], H, H, 0, P[CAMO_P_FU_W3], lo);
    }
    for (int lo = 0; lo < 2; ++lo) xheads(tp.Wh0[lo], 2 * H, H, 0, lo);
    if (pl.tail != CAMO_TAIL_PLANES)        // training calls: the transposed planes of the tail's backward (tail_wide.h, TailWideBwdArgs)
      for (int lo = 0; lo < 2; ++lo) {
        xheads(tp.Wh0T[lo], H, 2 * H, 1, lo);
        xj(tp.Wfu3T[lo], H, H, 1, P[CAMO_P_FU_W3], lo);
        xj(tp.Wfu0T[lo], 2 * H, H, 1, P[CAMO_P_FU_W0], lo);
        xj(tp.W13T[lo], 2 * H, H, 1, P[CAMO_P_F1_W3], lo);
        xj(tp.W23T[lo], 2 * H, H, 1, P[CAMO_P_F2_W3], lo);
      }
  }
  if (pl.front == CAMO_FRONT_KG) { fa.split3 = 1; CK(launch_wide_front(fa, 1, st, 1), "fused forward, KG rows' front half (32-row tiles, one in-projection pass per block)"); }
  else if (pl.front == CAMO_FRONT_WIDE) CK(launch_wide_front(fa, pl.front_rt, st, 0), "fused forward, front half (wide tiles)");
  else CK(launch_fused_front(fa, x.opt->fused_variant, st), "fused forward, front half");
  BackArgs ba; std::memset(&ba, 0, sizeof(ba));
  ba.s[0] = BackStream{sh.Wo1, P[CAMO_P_A1_OUT_B], sh.W1, P[CAMO_P_F1_B0], P[CAMO_P_LN1_W], P[CAMO_P_LN1_B], f.R16,
                       f.O16, f.Y16, f.XH16, f.rstd1, f.mask1, w.Ymean, w.H1mean, SITE_FFN_RG};
  ba.s[1] = BackStream{sh.Wo2, P[CAMO_P_A2_OUT_B], sh.W2, P[CAMO_P_F2_B0], P[CAMO_P_LN2_W], P[CAMO_P_LN2_B], f.G16,
                       f.O2_16, f.Y2_16, f.XH2_16, f.rstd2, f.mask2, w.Y2mean, w.H2mean, SITE_FFN_KG};
  ba.Q16 = f.Q16; ba.KV16 = f.KV16; ba.Q2_16 = f.Q2_16; ba.KV2_16 = f.KV2_16;
  ba.off = x.rg_offsets; ba.tile_off = x.bd.tile_off; ba.tile_desc = x.bd.tile_desc; ba.inv_nr = x.bd.inv_nr; ba.lse2 = f.lse2;
  ba.B = B; ba.Nk = Nk; ba.rows_rg = T; ba.rg_tiles_max = T / 32 + B;          // >= sum of ceil(Nr / 32); surplus blocks exit at once
  ba.part = f.part; ba.tickets = w.tickets; ba.max_splits = (max_nr + 63) / 64;
  ba.drop = x.drop; ba.save = save ? 1 : 0; ba.save_lse2 = pl.maps; ba.exp = x.opt->exp;
  ba.stamps = g_dbg_stamps ? g_dbg_stamps + (size_t)g_dbg_stamp_blocks * 8 : nullptr;
  switch (pl.back) {
    case CAMO_BACK_RG_64: CK(launch_wide2_rgfwd(fa.s[0], sh.Wf_rg, sh.bf_rg, fa.qscale, ba, max_nr, pl.save_r16, st), "fused forward, RG rows in one launch (64-row half-blocks)"); break;
    case CAMO_BACK_RG_WIDE: CK(launch_wide_rgfwd(fa.s[0], fa.qscale, ba, pl.back_rt, max_nr, st), "fused forward, RG rows in one launch (wide tiles)"); break;
    case CAMO_BACK_WIDE: CK(launch_wide_back(ba, pl.back_rt, max_nr, st), "fused forward, back half (wide tiles)"); break;
    default: CK(launch_fused_back(ba, x.opt->fused_variant, x.opt->back_lead, st), "fused forward, back half");
  }
  if (pl.maps) {
    // both head-averaged maps from what the two halves left in the workspace: one launch over the batch descriptor's tile table,
    // behind the back half (lse2) and independent of the per-sample tail
    AttnMapsArgs ma; std::memset(&ma, 0, sizeof(ma));
    ma.Q16 = f.Q16; ma.KV16 = f.KV16; ma.Q2_16 = f.Q2_16; ma.KV2_16 = f.KV2_16; ma.lse2 = f.lse2; ma.tile_desc = x.bd.tile_desc;
    ma.rg2kg = attn_rg2kg; ma.kg2rg = attn_kg2rg; ma.Nk = Nk; ma.tiles = T / 32 + B; ma.rows_rg = T;
    CK(launch_attn_maps(ma, st), "attention maps of the fused forward");
  }
  return 0;
}

// camo_forward_loss_backward's optional event: recorded on the stream as soon as the gradients of the per-sample tail (pooled
// FFN layers, fusion layer, heads: parameters CAMO_P_F2_W3 .. end of the table, and CAMO_P_F1_W3/B3) are final, so that a
// data-parallel caller can start reducing that part of the flat buffer while the node-level backward runs.  (camo_plan_t::tail_event
// names the one point of a call that records it.)
int record_tail_event(const Call& c, hipStream_t st) { return c.tail_event ? (int)hipEventRecord(c.tail_event, st) : 0; }

// ---- node-level backward of the bf16 schedule (w.dcomb, w.dHm1, w.dHm2 hold the pooled gradients) ----
int backward_nodes16(const Batch& x) {
  const camo_dims_t& d = *x.dims; const float* const* P = x.P; float* const* Gr = x.Gr; const Ws& w = x.w; const DropCfg& drop = x.drop; hipStream_t st = x.st;
  const int32_t* rg_offsets = x.rg_offsets; const int32_t* row_sample = x.bd.row_sample; const float* inv_nr = x.bd.inv_nr;
  const int B = x.B, T = x.T, Nk = x.Nk;
  const int H = d.hidden_dim, D = d.rg_dim, Dk = d.kg_dim, TK = B * Nk, nh = d.num_heads;
  const size_t HH = (size_t)H * H;
  const Ws::H16& h = w.h;
  // dH1 = mask(H1) * bcast(dHm1) / n is needed only as a GEMM operand.  At hidden_dim 256 and B <= 32 the whole-row
  // kernel builds it while staging (GF_A_VIRT) from the bf16 activation mask and the per-sample gradient rows, for both
  // products that read it; otherwise relu_bcast_bwd writes it out.
  const bool virt = H == 256 && B <= 32;
  if (!virt) {
    BcastSeg s0{nullptr, w.dHm1, 2 * H, row_sample, inv_nr, 0, nullptr, T, h.dH1, h.H1};
    BcastSeg s1{nullptr, w.dHm2, 2 * H, nullptr, nullptr, Nk, nullptr, TK, h.dH2, h.H2};
    CK(launch_relu_bcast_bwd(s0, s1, 2 * H, drop.scale, st), "relu bcast bwd");
  }
  auto make_virt = [&](Gemm16Prob& p, const float* g_rows, bool rg_side) {
    p.flags |= GF_A_VIRT; p.virt_g = g_rows; p.ldg = 2 * H; p.aux_scale = drop.scale;
    if (rg_side) { p.row_sample = row_sample; p.inv_nr = inv_nr; p.uniform_n = 0; } else { p.row_sample = nullptr; p.inv_nr = nullptr; p.uniform_n = Nk; }
    if (p.flags & GF_A_KMAJOR) p.ldc16 = B;               // (sample count of a weight-gradient problem)
  };
  GB16 g(drop, *x.opt, st);
  // first FFN layer: dY = bcast(dpool)/n + dH1.W1 ; dW1 += dH1^T.Y -- and, at hidden_dim 256, the LayerNorm backward
  // dY -> dU (+ dgamma, dbeta) as the epilogue of the dY product (whole-row tiles)
  if (H == 256) {
    Gemm16Prob& p1 = g.nt(virt ? h.H1 : h.dH1, 2 * H, h.W1T, 2 * H, nullptr, w.dU, H, h.dU, H, T, H, 2 * H);
    set_bcast(p1, w.dcomb, 2 * H, row_sample, inv_nr, 0);
    p1.ln_mode = 2; p1.ln_gamma = P[CAMO_P_LN1_W]; p1.ln_stats = w.st1; p1.ln_x = w.U;
    p1.ln_dgamma = Gr[CAMO_P_LN1_W]; p1.ln_dbeta = Gr[CAMO_P_LN1_B];
    if (virt) make_virt(p1, w.dHm1, true);
    Gemm16Prob& p2 = g.nt(virt ? h.H2 : h.dH2, 2 * H, h.W2T, 2 * H, nullptr, w.dU2, H, h.dU2, H, TK, H, 2 * H);
    set_bcast(p2, w.dcomb + H, 2 * H, nullptr, nullptr, Nk);
    p2.ln_mode = 2; p2.ln_gamma = P[CAMO_P_LN2_W]; p2.ln_stats = w.st2; p2.ln_x = w.U2;
    p2.ln_dgamma = Gr[CAMO_P_LN2_W]; p2.ln_dbeta = Gr[CAMO_P_LN2_B];
    if (virt) make_virt(p2, w.dHm2, false);
  } else {
    set_bcast(g.nt(h.dH1, 2 * H, h.W1T, 2 * H, nullptr, w.dY, H, nullptr, 0, T, H, 2 * H), w.dcomb, 2 * H, row_sample, inv_nr, 0);
    set_bcast(g.nt(h.dH2, 2 * H, h.W2T, 2 * H, nullptr, w.dY2, H, nullptr, 0, TK, H, 2 * H), w.dcomb + H, 2 * H, nullptr, nullptr, Nk);
  }
  {
    Gemm16Prob& t1 = g.tn(virt ? h.H1 : h.dH1, 2 * H, h.Y, H, Gr[CAMO_P_F1_W0], H, Gr[CAMO_P_F1_B0], 2 * H, H, T);
    if (virt) make_virt(t1, w.dHm1, true);
    Gemm16Prob& t2 = g.tn(virt ? h.H2 : h.dH2, 2 * H, h.Y2, H, Gr[CAMO_P_F2_W0], H, Gr[CAMO_P_F2_B0], 2 * H, H, TK);
    if (virt) make_virt(t2, w.dHm2, false);
  }
  CK(g.run(), "ffn layer 0 bwd");
  if (H != 256) {
    LnBwdSeg s0{w.U, w.dY, w.st1, P[CAMO_P_LN1_W], w.dU, Gr[CAMO_P_LN1_W], Gr[CAMO_P_LN1_B], T, h.dU};
    LnBwdSeg s1{w.U2, w.dY2, w.st2, P[CAMO_P_LN2_W], w.dU2, Gr[CAMO_P_LN2_W], Gr[CAMO_P_LN2_B], TK, h.dU2};
    CK(launch_ln_bwd(s0, s1, H, st), "layernorm bwd");
  }
  // out-projections
  g.nt(h.dU, H, h.Wo1T, H, nullptr, w.dO, H, nullptr, 0, T, H, H);
  g.nt(h.dU2, H, h.Wo2T, H, nullptr, w.dO2, H, nullptr, 0, TK, H, H);
  g.tn(h.dU, H, h.O, H, Gr[CAMO_P_A1_OUT_W], H, Gr[CAMO_P_A1_OUT_B], H, H, T);
  g.tn(h.dU2, H, h.O2, H, Gr[CAMO_P_A2_OUT_W], H, Gr[CAMO_P_A2_OUT_B], H, H, TK);
  CK(g.run(), "out-projection bwd");
  // attention cores.  Their node-side outputs are GEMM operands only, so they are written as bf16 straight into the
  // concatenated [dQ | dK2 | dV2] (rg rows) and [dQ2 | dK | dV] (kg rows) operands of the in-projection backward.
  // Both directions run in one launch, each (head, sample) owned by one block, so nothing is accumulated with atomics.
  CK(launch_attn_bwd_pair(w.Q, w.KV, w.P, w.dO, w.Q2, w.KV2, w.P2, w.dO2, rg_offsets, Bf16Dst{h.dQKV, 3 * H},
                          Bf16Dst{h.dQKVkg + H, 3 * H}, Bf16Dst{h.dQKVkg, 3 * H}, Bf16Dst{h.dQKV + H, 3 * H}, w.O2, B, H, nh, Nk, drop, st),
     "attention bwd (both directions)");
  // in-projections: one K = 3H product per side for the input gradient (dR = dU + [dQ|dK2|dV2].[Wq1;Wk2;Wv2]),
  // and the four weight gradients
  set_res(g.nt(h.dQKV, 3 * H, h.WcRgT, 3 * H, nullptr, nullptr, 0, h.dR, H, T, H, 3 * H), w.dU, H);
  set_res(g.nt(h.dQKVkg, 3 * H, h.WcKgT, 3 * H, nullptr, nullptr, 0, h.dG, H, TK, H, 3 * H), w.dU2, H);
  CK(g.run(), "in-projection bwd (input gradients)");
  // every remaining weight gradient in one launch: the in-projection ones do not wait for dR / dG, but beside the
  // K = 3H products above they set that launch's length, while the lone dW_rg / dW_kg launch left most CUs idle
  g.tn(h.dQKV, 3 * H, h.R, H, Gr[CAMO_P_A1_IN_W], H, Gr[CAMO_P_A1_IN_B], H, H, T);
  g.tn(h.dQKV + H, 3 * H, h.R, H, Gr[CAMO_P_A2_IN_W] + HH, H, Gr[CAMO_P_A2_IN_B] + H, 2 * H, H, T);
  g.tn(h.dQKVkg, 3 * H, h.G, H, Gr[CAMO_P_A2_IN_W], H, Gr[CAMO_P_A2_IN_B], H, H, TK);
  g.tn(h.dQKVkg + H, 3 * H, h.G, H, Gr[CAMO_P_A1_IN_W] + HH, H, Gr[CAMO_P_A1_IN_B] + H, 2 * H, H, TK);
  g.tn(h.dR, H, h.X, D, Gr[CAMO_P_RG_PROJ_W], D, Gr[CAMO_P_RG_PROJ_B], H, D, T);
  g.tn(h.dG, H, h.KG, Dk, Gr[CAMO_P_KG_PROJ_W], Dk, Gr[CAMO_P_KG_PROJ_B], H, Dk, TK);
  CK(g.run(), "in-projection and input-projection weight gradients");
  return 0;
}

// the per-sample tail of the fused schedule as one launch (misc.hip, tail_fused_kernel); fl == null: forward only
int tail17(Call& c, const Batch& x, float* outs, const FusedLoss* fl) {
  const camo_dims_t& d = *x.dims; const float* const* P = x.P; float* const* Gr = x.Gr; const Ws& w = x.w; hipStream_t st = x.st;
  const int B = x.B;
  TailFusedArgs a; std::memset(&a, 0, sizeof(a));
  a.Ymean = w.Ymean; a.H1mean = w.H1mean; a.Y2mean = w.Y2mean; a.H2mean = w.H2mean;
  a.W13 = P[CAMO_P_F1_W3]; a.b13 = P[CAMO_P_F1_B3]; a.W23 = P[CAMO_P_F2_W3]; a.b23 = P[CAMO_P_F2_B3];
  a.Wfu0 = P[CAMO_P_FU_W0]; a.bfu0 = P[CAMO_P_FU_B0]; a.Wfu3 = P[CAMO_P_FU_W3]; a.bfu3 = P[CAMO_P_FU_B3];
  for (int x = 0; x < 4; ++x) {
    a.Wh0[x] = P[CAMO_P_HEADS + 4 * x]; a.bh0[x] = P[CAMO_P_HEADS + 4 * x + 1]; a.Wh3[x] = P[CAMO_P_HEADS + 4 * x + 2]; a.bh3[x] = P[CAMO_P_HEADS + 4 * x + 3];
  }
  if (fl) {
    a.gW13 = Gr[CAMO_P_F1_W3]; a.gb13 = Gr[CAMO_P_F1_B3]; a.gW23 = Gr[CAMO_P_F2_W3]; a.gb23 = Gr[CAMO_P_F2_B3];
    a.gWfu0 = Gr[CAMO_P_FU_W0]; a.gbfu0 = Gr[CAMO_P_FU_B0]; a.gWfu3 = Gr[CAMO_P_FU_W3]; a.gbfu3 = Gr[CAMO_P_FU_B3];
    for (int x = 0; x < 4; ++x) {
      a.gWh0[x] = Gr[CAMO_P_HEADS + 4 * x]; a.gbh0[x] = Gr[CAMO_P_HEADS + 4 * x + 1]; a.gWh3[x] = Gr[CAMO_P_HEADS + 4 * x + 2]; a.gbh3[x] = Gr[CAMO_P_HEADS + 4 * x + 3];
    }
    a.y = reinterpret_cast<const long long*>(fl->y); a.e = fl->e; a.s = fl->s; a.terms = fl->terms; a.pred = fl->pred;
    a.dcomb = w.dcomb; a.dHm1 = w.dHm1; a.dHm2 = w.dHm2;
  }
  a.outs = outs;
  a.F1sum = w.tailsum.F1sum; a.hidsum = w.tailsum.hidsum; a.dF1sum = w.tailsum.dF1sum; a.counters = w.tailsum.counters;
  a.B = B; a.C = d.num_classes; a.mode = fl ? 1 : 0; a.drop = x.drop;
  a.stamps = g_dbg_stamps ? g_dbg_stamps + (size_t)4 * g_dbg_stamp_blocks * 8 : nullptr;
  a.debug_skip = c.tail_skip;
  // training: the kernel leaves copies of the operands of the eight big weight gradients (for_tail_wg), and these gradients to the
  // launches behind it: nothing on the chain to the node-level backward waits for them
  if (fl) { a.comb_out = w.comb; a.F1_out = w.F1; a.fused_out = w.fused; a.dhid_out = w.dhid; a.dfused_out = w.dfused; a.dF1_out = w.dF1; }
  CK(launch_tail_fused(a, st), "per-sample tail (one launch)");
  c.tail_skip_taken = a.debug_skip != 0;
  if (x.plan.tail_wg == CAMO_TAIL_WG_LAUNCH) {      // (operands = the copies the tail kernel left in the workspace)
    GB g(x.drop, 0, st);
    add_tail_wg(x, g);
    CK(g.run(), "per-sample tail, weight gradients");
  }
  return 0;
}

// the per-sample tail's forward as the one two-plane launch (tail_wide.h), behind a front launch that built its weight planes
int tail_planes_forward(const Batch& x, float* outs, const FusedLoss* fl) {
  const camo_dims_t& d = *x.dims; const float* const* P = x.P; const Ws& w = x.w;
  const bool train = x.plan.tail != CAMO_TAIL_PLANES;
  TailWideArgs ta; std::memset(&ta, 0, sizeof(ta));
  ta.Ymean = w.Ymean; ta.H1mean = w.H1mean; ta.Y2mean = w.Y2mean; ta.H2mean = w.H2mean;
  const Ws::F17::TailPlanes& tp = w.f.tp;
  ta.T13h = tp.W13.hi; ta.T13l = tp.W13.lo; ta.T23h = tp.W23.hi; ta.T23l = tp.W23.lo; ta.Tfu0h = tp.Wfu0.hi; ta.Tfu0l = tp.Wfu0.lo;
  ta.Tfu3h = tp.Wfu3.hi; ta.Tfu3l = tp.Wfu3.lo; ta.Th0h = tp.Wh0.hi; ta.Th0l = tp.Wh0.lo;
  ta.b13 = P[CAMO_P_F1_B3]; ta.b23 = P[CAMO_P_F2_B3]; ta.bfu0 = P[CAMO_P_FU_B0]; ta.bfu3 = P[CAMO_P_FU_B3];
  for (int x = 0; x < 4; ++x) { ta.bh0[x] = P[CAMO_P_HEADS + 4 * x + 1]; ta.Wh3[x] = P[CAMO_P_HEADS + 4 * x + 2]; ta.bh3[x] = P[CAMO_P_HEADS + 4 * x + 3]; }
  ta.outs = outs; ta.B = x.B; ta.C = d.num_classes; ta.drop = x.drop;
  if (train) { ta.comb_out = w.comb; ta.F1_out = w.F1; ta.fused_out = w.fused; ta.hid_out = w.hid; }
  CK(launch_tail_wide(ta, x.st), "per-sample tail (wide, one launch)");
  if (!train) return 0;
  // (the output layers' weight gradients ride in the tail's weight-gradient launch of the backward half, when that half takes it)
  return heads_forward(x, CAMO_P_HEADS, d.hidden_dim, outs, fl, /*hidden_done=*/true, /*defer_out_grads=*/x.plan.tail == CAMO_TAIL_PLANES_TRAIN);
}

// ... and its backward: the tail's input-gradient chain as ONE two-plane launch + ONE launch for its weight gradients
int tail_planes_backward(const Batch& x) {
  const camo_dims_t& d = *x.dims; float* const* Gr = x.Gr; const Ws& w = x.w;
  const int H = d.hidden_dim, B = x.B;
  TailWideBwdArgs ta; std::memset(&ta, 0, sizeof(ta));
  const Ws::F17::TailPlanes& tp = w.f.tp;
  ta.dhid = w.dhid; ta.F1 = w.F1;
  ta.Th0h = tp.Wh0T.hi; ta.Th0l = tp.Wh0T.lo; ta.Tfu3h = tp.Wfu3T.hi; ta.Tfu3l = tp.Wfu3T.lo; ta.Tfu0h = tp.Wfu0T.hi; ta.Tfu0l = tp.Wfu0T.lo;
  ta.T13h = tp.W13T.hi; ta.T13l = tp.W13T.lo; ta.T23h = tp.W23T.hi; ta.T23l = tp.W23T.lo;
  ta.dfused = w.dfused; ta.dF1 = w.dF1; ta.dcomb = w.dcomb; ta.dHm1 = w.dHm1; ta.dHm2 = w.dHm2;
  ta.B = B; ta.scale = x.drop.scale;
  CK(launch_tail_wide_bwd(ta, x.st), "per-sample tail, input gradients (wide, one launch)");
  const int Fh = H / 2, C = d.num_classes, Wd = 2 * C + 2, nout[4] = {C, C, 1, 1}, coff[4] = {0, C, 2 * C, 2 * C + 1};
  float* const* hg = Gr + CAMO_P_HEADS;
  GB gt = tail_gemms(x);
  for (int h = 0; h < 4; ++h) gt.tn(w.dlog + coff[h], Wd, w.hid + h * Fh, 4 * Fh, hg[4 * h + 2], Fh, hg[4 * h + 3], nout[h], Fh, B);   // (left by the loss launch)
  add_tail_wg(x, gt);
  CK(gt.run(), "per-sample tail, weight gradients");
  return 0;
}

// ---- node-level backward of the fused row-tile schedule (w.dcomb, w.dHm1, w.dHm2 hold the pooled gradients) ----
int backward_nodes17(Call& c, const Batch& x) {
  const camo_plan_t& pl = x.plan; const float* const* P = x.P; float* const* Gr = x.Gr; const Ws& w = x.w; const DropCfg& drop = x.drop; hipStream_t st = x.st;
  const int32_t* rg_offsets = x.rg_offsets; const Desc& bd = x.bd;
  const int H = 256, D = 128, B = x.B, T = x.T, Nk = x.Nk, TK = B * Nk;
  const size_t HH = (size_t)H * H;
  const Ws::F17& f = w.f; const ShadowSet& sh = f.sh;
  Bwd1Args a1; std::memset(&a1, 0, sizeof(a1));
  a1.s[0] = Bwd1Stream{sh.W1T, sh.Wo1T, f.mask1, f.XH16, f.rstd1, P[CAMO_P_LN1_W], w.dHm1, 2 * H, w.dcomb, 2 * H, f.dH16, f.dU16,
                       Gr[CAMO_P_LN1_W], Gr[CAMO_P_LN1_B]};
  a1.s[1] = Bwd1Stream{sh.W2T, sh.Wo2T, f.mask2, f.XH2_16, f.rstd2, P[CAMO_P_LN2_W], w.dHm2, 2 * H, w.dcomb + H, 2 * H, f.dH2_16, f.dU2_16,
                       Gr[CAMO_P_LN2_W], Gr[CAMO_P_LN2_B]};
  a1.Q16 = f.Q16; a1.KV16 = f.KV16; a1.dQKV16 = f.dQKV16; a1.dKV = w.dKV;
  a1.O2_16 = f.O2_16; a1.dO2_16 = f.dO2_16; a1.delta2 = f.delta2;
  a1.off = rg_offsets; a1.tile_off = bd.tile_off; a1.tile_desc = bd.tile_desc; a1.inv_nr = bd.inv_nr; a1.row_sample = bd.row_sample;
  a1.B = B; a1.Nk = Nk; a1.rows_rg = T; a1.rg_tiles_max = T / 32 + B; a1.qscale = 1.0f / sqrtf(32.0f); a1.drop = drop;
  a1.stamps = g_dbg_stamps ? g_dbg_stamps + (size_t)2 * g_dbg_stamp_blocks * 8 : nullptr;
  a1.nzero = c.nzero_bwd1; a1.exp = x.opt->exp;
  // per-block slabs instead of atomics for dK | dV and the LayerNorm sums: by size (the launcher's rule), where the second half is the kernel that sums them
  a1.slabKV = f.slabKV; a1.slabLN = f.slabLN; a1.max_nr = x.max_nr;
  a1.slabs = (pl.bwd1 == CAMO_BWD1_ROWS32 && pl.bwd2 == CAMO_BWD2_ROWS32 && pl.param_space == 0) ? -1 : 0;
  for (int i = 0; i < c.nzero_bwd1; ++i) { a1.zero_ptr[i] = c.zero_bwd1_ptr[i]; a1.zero_bytes[i] = c.zero_bwd1_bytes[i]; }
  if (pl.tail_wg == CAMO_TAIL_WG_BWD1) {
    // the one-launch tail's eight big weight gradients (tail17), from the operand copies it left
    TailWgArgs& t = a1.twg;
    for_tail_wg(x, [&](const float* dy, int ld_dy, const float* xin, int ld_x, float* dW, float* db, int rows, int cols) {
      t.p[t.n++] = TailWgProd{dy, xin, dW, db, ld_dy, ld_x, rows, cols, 0};
    });
    t.B = B;
  }
  if (pl.bwd1 == CAMO_BWD1_64) CK(launch_wide2_bwd1(a1, x.opt->fused_variant, st), "fused backward, first half (64-row half-blocks)");
  else                         CK(launch_fused_bwd1(a1, x.opt->fused_variant, st), "fused backward, first half");
  if (pl.tail_event == CAMO_EVENT_AFTER_BWD1) CK(record_tail_event(c, st), "tail event");      // (the one-launch tail's weight gradients are final behind the launch above)
  Bwd2Args a2; std::memset(&a2, 0, sizeof(a2));
  a2.Q2_16 = f.Q2_16; a2.dO2_16 = f.dO2_16; a2.lse2 = f.lse2; a2.delta2 = f.delta2; a2.KV2_16 = f.KV2_16; a2.dQKV16 = f.dQKV16;
  a2.dU16 = f.dU16; a2.WcRgT = sh.WcRgT; a2.dR16 = f.dR16; a2.dQ2acc = w.dQ2acc; a2.dKV = w.dKV;
  a2.slabs = a1.slabs; a2.slabKV = f.slabKV; a2.slabLN = f.slabLN;
  for (int i = 0; i < 2; ++i) { a2.ln_dgamma[i] = a1.s[i].dgamma; a2.ln_dbeta[i] = a1.s[i].dbeta; }
  a2.dU2_16 = f.dU2_16; a2.WcKgT = sh.WcKgT; a2.dQKVkg16 = f.dQKVkg16; a2.dG16 = f.dG16; a2.dGpart = f.dGpart;
  a2.tickets = w.tickets + B; a2.off = rg_offsets; a2.tile_off = bd.tile_off; a2.tile_desc = bd.tile_desc;
  a2.B = B; a2.Nk = Nk; a2.rows_rg = T; a2.rg_tiles_max = T / 32 + B; a2.qscale = a1.qscale; a2.drop = drop;
  a2.stamps = g_dbg_stamps ? g_dbg_stamps + (size_t)3 * g_dbg_stamp_blocks * 8 : nullptr;
  const bool param_space = pl.param_space != 0;
  a2.param_space = param_space ? 1 : 0;
  a2.split_finish = pl.bwd2 != CAMO_BWD2_ROWS32 ? 1 : 0;
  // row space: the KG rows' dQ2 chain finishes in the weight-gradient launch when the launcher finds B Nk small enough (it leaves its
  // choice in kg_defer).  Developer A/B: exp = 32 keeps the arrival protocol in bwd2, exp = 64 defers at any size.  A forced tn_big keeps
  // it too: the 128 x 256 weight-gradient kernel takes bf16 operands only, and forcing it is an A/B of the two kernels on one operand set
  a2.kg_defer = x.opt->exp == 32 ? 0 : (x.opt->exp == 64 ? 1 : (x.opt->tn_big > 0 ? 0 : -1));
  if (pl.bwd2 == CAMO_BWD2_64) CK(launch_wide2_bwd2(a2, st), "fused backward, second half (64-row blocks)");
  else CK(launch_fused_bwd2(a2, x.opt->fused_variant, st), "fused backward, second half");
  // every node-level weight gradient: dW += dy^T . x over the rows of a stream (bf16 operands the fused kernels wrote)
  if (!param_space) {
    GB16 g(drop, *x.opt, st);
    const bool kgq = a2.kg_defer == 1;
    if (kgq) {
      // first in the launch: dW_kgproj += Wq2^T (dQ2^T KG), db_kgproj += Wq2^T colsum(dQ2) -- the part of dG^T KG that bwd2 left out of its operand (dGpart)
      Gemm16Prob& p = g.tn(nullptr, H, f.KG16, D, Gr[CAMO_P_KG_PROJ_W], D, Gr[CAMO_P_KG_PROJ_B], H, D, TK);
      p.A = reinterpret_cast<const us*>(w.dQ2acc); p.flags |= GF_A_F32 | GF_KGQ;
      p.kgq_wT = sh.WcKgT; p.kgq_w = P[CAMO_P_A2_IN_W]; p.ldg = H;
      // (the workspace's record: dG16 and the dQ2 columns of dQKVkg16, which nothing in this launch reads)
      p.C16 = f.dG16; p.ldc16 = H; p.kgq_part16 = reinterpret_cast<const us*>(f.dGpart); p.kgq_a16 = f.dQKVkg16; p.kgq_lda16 = 3 * H;
    }
    g.tn(f.dH16, 2 * H, f.Y16, H, Gr[CAMO_P_F1_W0], H, Gr[CAMO_P_F1_B0], 2 * H, H, T);
    g.tn(f.dU16, H, f.O16, H, Gr[CAMO_P_A1_OUT_W], H, Gr[CAMO_P_A1_OUT_B], H, H, T);
    g.tn(f.dQKV16, 3 * H, f.R16, H, Gr[CAMO_P_A1_IN_W], H, Gr[CAMO_P_A1_IN_B], H, H, T);
    g.tn(f.dQKV16 + H, 3 * H, f.R16, H, Gr[CAMO_P_A2_IN_W] + HH, H, Gr[CAMO_P_A2_IN_B] + H, 2 * H, H, T);
    g.tn(f.dR16, H, f.X16, D, Gr[CAMO_P_RG_PROJ_W], D, Gr[CAMO_P_RG_PROJ_B], H, D, T);
    g.tn(f.dH2_16, 2 * H, f.Y2_16, H, Gr[CAMO_P_F2_W0], H, Gr[CAMO_P_F2_B0], 2 * H, H, TK);
    g.tn(f.dU2_16, H, f.O2_16, H, Gr[CAMO_P_A2_OUT_W], H, Gr[CAMO_P_A2_OUT_B], H, H, TK);
    if (kgq) {     // the q rows of attn2.in_proj from the fp32 dQ2 sums: their bf16 columns of dQKVkg16 are only being written by this launch
      Gemm16Prob& p = g.tn(nullptr, H, f.G16, H, Gr[CAMO_P_A2_IN_W], H, Gr[CAMO_P_A2_IN_B], H, H, TK);
      p.A = reinterpret_cast<const us*>(w.dQ2acc); p.flags |= GF_A_F32;
    } else {
      g.tn(f.dQKVkg16, 3 * H, f.G16, H, Gr[CAMO_P_A2_IN_W], H, Gr[CAMO_P_A2_IN_B], H, H, TK);
    }
    g.tn(f.dQKVkg16 + H, 3 * H, f.G16, H, Gr[CAMO_P_A1_IN_W] + HH, H, Gr[CAMO_P_A1_IN_B] + H, 2 * H, H, TK);
    g.tn(kgq ? reinterpret_cast<const us*>(f.dGpart) : f.dG16, H, f.KG16, D, Gr[CAMO_P_KG_PROJ_W], D, Gr[CAMO_P_KG_PROJ_B], H, D, TK);
    CK(g.run(), "node-level weight gradients");
    return 0;
  }
  // Node-level weight gradients: dW += dy^T . x over the rows of a stream (bf16 operands the fused kernels wrote).  The input
  // projection and the in-projections take theirs in PARAMETER space -- with R = x W_p^T + b_p and [q|k'|v'] = R W_in^T + b_in:
  //   M = dQKV^T x  [3H][D],  db_in = colsum(dQKV);   dW_in = dQKV^T R = M W_p^T + db_in b_p^T;
  //   dW_p = dR^T x = dU^T x + W_in^T M,  db_p = colsum(dU) + W_in^T db_in      (dR = dU + dQKV W_in never exists)
  // -- 131 k MACs per row (M, dU^T x) instead of 427 k (dR, dQKV^T R, dR^T x), and one small fp32 launch behind them (misc.hip, unfold_kernel).
  float* const Mrg = w.parM.Mrg; float* const Mkg = w.parM.Mkg; float* const dbrg = w.parM.dbrg; float* const dbkg = w.parM.dbkg;
  GB16 g(drop, *x.opt, st);
  g.tn(f.dH16, 2 * H, f.Y16, H, Gr[CAMO_P_F1_W0], H, Gr[CAMO_P_F1_B0], 2 * H, H, T);
  g.tn(f.dU16, H, f.O16, H, Gr[CAMO_P_A1_OUT_W], H, Gr[CAMO_P_A1_OUT_B], H, H, T);
  g.tn(f.dQKV16, 3 * H, f.X16, D, Mrg, D, dbrg, H, D, T).bias_grad2 = Gr[CAMO_P_A1_IN_B];
  g.tn(f.dQKV16 + H, 3 * H, f.X16, D, Mrg + (size_t)H * D, D, dbrg + H, 2 * H, D, T).bias_grad2 = Gr[CAMO_P_A2_IN_B] + H;
  g.tn(f.dU16, H, f.X16, D, Gr[CAMO_P_RG_PROJ_W], D, Gr[CAMO_P_RG_PROJ_B], H, D, T);
  g.tn(f.dH2_16, 2 * H, f.Y2_16, H, Gr[CAMO_P_F2_W0], H, Gr[CAMO_P_F2_B0], 2 * H, H, TK);
  g.tn(f.dU2_16, H, f.O2_16, H, Gr[CAMO_P_A2_OUT_W], H, Gr[CAMO_P_A2_OUT_B], H, H, TK);
  g.tn(f.dQKVkg16, 3 * H, f.KG16, D, Mkg, D, dbkg, H, D, TK).bias_grad2 = Gr[CAMO_P_A2_IN_B];
  g.tn(f.dQKVkg16 + H, 3 * H, f.KG16, D, Mkg + (size_t)H * D, D, dbkg + H, 2 * H, D, TK).bias_grad2 = Gr[CAMO_P_A1_IN_B] + H;
  g.tn(f.dU2_16, H, f.KG16, D, Gr[CAMO_P_KG_PROJ_W], D, Gr[CAMO_P_KG_PROJ_B], H, D, TK);
  CK(g.run(), "node-level weight gradients");
  {
    const UnfoldStream urg{Mrg, dbrg, P[CAMO_P_A1_IN_W], P[CAMO_P_A2_IN_W] + HH, P[CAMO_P_RG_PROJ_W], P[CAMO_P_RG_PROJ_B], Gr[CAMO_P_A1_IN_W],
                           Gr[CAMO_P_A2_IN_W] + HH, Gr[CAMO_P_RG_PROJ_W], Gr[CAMO_P_RG_PROJ_B]};
    const UnfoldStream ukg{Mkg, dbkg, P[CAMO_P_A2_IN_W], P[CAMO_P_A1_IN_W] + HH, P[CAMO_P_KG_PROJ_W], P[CAMO_P_KG_PROJ_B], Gr[CAMO_P_A2_IN_W],
                           Gr[CAMO_P_A1_IN_W] + HH, Gr[CAMO_P_KG_PROJ_W], Gr[CAMO_P_KG_PROJ_B]};
    CK(launch_unfold(urg, ukg, st), "projection / in-projection weight gradients (parameter space)");
  }
  return 0;
}

// ---- LateFusion.forward, fusion_model.py:164-171
int forward_late(const Batch& x, float* outs, const FusedLoss* fl) {
  const camo_dims_t& d = *x.dims; const float* const* P = x.P; const Ws& w = x.w; hipStream_t st = x.st;
  const int H = d.hidden_dim, D = d.rg_dim, Dk = d.kg_dim, B = x.B, Nk = x.Nk, F = H / 2, Dc = D + Dk;
  CK((int)hipMemsetAsync(w.zero_base, 0, w.zero_bytes, st), "memset zero block");
  GB gt = tail_gemms(x);
  SegMean sm[2] = {{x.rg, D, D, x.rg_offsets, 0, w.comb, Dc}, {x.kg, Dk, Dk, nullptr, Nk, w.comb + D, Dc}};
  CK(launch_seg_mean(sm, 2, B, x.max_nr > Nk ? x.max_nr : Nk, st), "late means");
  set_drop(gt.nt(w.comb, Dc, P[CAMO_PL_W0], Dc, P[CAMO_PL_B0], w.F1, H, B, H, Dc, GF_RELU), SITE_LATE0);
  CK(gt.run(), "late fc0");
  set_drop(gt.nt(w.F1, H, P[CAMO_PL_W3], H, P[CAMO_PL_B3], w.a2, F, B, F, H, GF_RELU), SITE_LATE0 + 1);
  CK(gt.run(), "late fc3");
  gt.nt(w.a2, F, P[CAMO_PL_W6], F, P[CAMO_PL_B6], w.fused, F, B, F, F);
  CK(gt.run(), "late fc6");
  return heads_forward(x, CAMO_PL_HEADS, F, outs, fl);
}

int backward_late(const Batch& x, const float* outs, const float* d_outs, int pre_activation, bool heads_out_done) {
  const camo_dims_t& d = *x.dims; const float* const* P = x.P; float* const* Gr = x.Gr; const Ws& w = x.w; const DropCfg& drop = x.drop;
  const int H = d.hidden_dim, B = x.B, F = H / 2, Dc = d.rg_dim + d.kg_dim;
  if (int e = heads_backward(x, CAMO_PL_HEADS, F, outs, d_outs, pre_activation, heads_out_done)) return e;
  GB gt = tail_gemms(x);
  set_relu_bwd(gt.nn(w.dfused, F, P[CAMO_PL_W6], F, w.da2, F, B, F, F), w.a2, F, drop.scale);
  gt.tn(w.dfused, F, w.a2, F, Gr[CAMO_PL_W6], F, Gr[CAMO_PL_B6], F, F, B);
  CK(gt.run(), "late fc6 bwd");
  set_relu_bwd(gt.nn(w.da2, F, P[CAMO_PL_W3], H, w.dF1, H, B, H, F), w.F1, H, drop.scale);
  gt.tn(w.da2, F, w.F1, H, Gr[CAMO_PL_W3], H, Gr[CAMO_PL_B3], F, H, B);
  CK(gt.run(), "late fc3 bwd");
  gt.tn(w.dF1, H, w.comb, Dc, Gr[CAMO_PL_W0], Dc, Gr[CAMO_PL_B0], H, Dc, B);
  CK(gt.run(), "late fc0 bwd");
  return 0;
}

// ---- node-level forward of the general schedule (fp32 operands, any configuration): CrossAttentionFusion.forward, fusion_model.py:75-135
int forward_nodes_general(const Batch& x, float* attn_rg2kg, float* attn_kg2rg) {
  const camo_dims_t& d = *x.dims; const float* const* P = x.P; const Ws& w = x.w; const DropCfg& drop = x.drop; hipStream_t st = x.st;
  const float* rg = x.rg; const float* kg = x.kg; const int32_t* rg_offsets = x.rg_offsets;
  const int H = d.hidden_dim, D = d.rg_dim, Dk = d.kg_dim, B = x.B, T = x.T, Nk = x.Nk, TK = B * Nk, nh = d.num_heads, max_nr = x.max_nr;
  const size_t HH2 = (size_t)H * H;
  // one clear of everything this step accumulates into with atomics (means now, dfused/dKV in backward);
  // the other schedules' first launch does it along with its casts / shadows
  CK((int)hipMemsetAsync(w.zero_base, 0, w.zero_bytes, st), "memset zero block");
  GB g(drop, x.precision, st);
  const float* R = rg; const float* G = kg;
  if (P[CAMO_P_KG_PROJ_W]) { g.nt(kg, Dk, P[CAMO_P_KG_PROJ_W], Dk, P[CAMO_P_KG_PROJ_B], w.G, H, TK, H, Dk); G = w.G; }
  if (P[CAMO_P_RG_PROJ_W]) { g.nt(rg, D, P[CAMO_P_RG_PROJ_W], D, P[CAMO_P_RG_PROJ_B], w.R, H, T, H, D); R = w.R; }
  CK(g.run(), "input projections");
  // in-projections of both attention blocks (packed in_proj_weight: rows 0..H-1 = Wq, H..3H-1 = Wk|Wv)
  g.nt(R, H, P[CAMO_P_A1_IN_W], H, P[CAMO_P_A1_IN_B], w.Q, H, T, H, H);
  g.nt(R, H, P[CAMO_P_A2_IN_W] + HH2, H, P[CAMO_P_A2_IN_B] + H, w.KV2, 2 * H, T, 2 * H, H);
  g.nt(G, H, P[CAMO_P_A1_IN_W] + HH2, H, P[CAMO_P_A1_IN_B] + H, w.KV, 2 * H, TK, 2 * H, H);
  g.nt(G, H, P[CAMO_P_A2_IN_W], H, P[CAMO_P_A2_IN_B], w.Q2, H, TK, H, H);
  CK(g.run(), "attention in-projections");
  CK(launch_attn_rg2kg_fwd(w.Q, w.KV, rg_offsets, w.P, w.O, attn_rg2kg, B, T, max_nr, H, nh, Nk, drop, st), "attn rg2kg fwd");
  CK(launch_attn_kg2rg_fwd(w.Q2, w.KV2, rg_offsets, w.P2, w.O2, B, max_nr, H, nh, Nk, drop, st), "attn kg2rg fwd");
  if (attn_kg2rg) CK(launch_attn_avg(w.P2, attn_kg2rg, T, nh, Nk, drop, st), "attn avg");
  // out-projection + residual (fusion_model.py:119,130), then LayerNorm
  set_res(g.nt(w.O, H, P[CAMO_P_A1_OUT_W], H, P[CAMO_P_A1_OUT_B], w.U, H, T, H, H), R, H);
  set_res(g.nt(w.O2, H, P[CAMO_P_A2_OUT_W], H, P[CAMO_P_A2_OUT_B], w.U2, H, TK, H, H), G, H);
  CK(g.run(), "attention out-projections");
  {
    LnSeg s0{w.U, w.Y, w.st1, P[CAMO_P_LN1_W], P[CAMO_P_LN1_B], T};
    LnSeg s1{w.U2, w.Y2, w.st2, P[CAMO_P_LN2_W], P[CAMO_P_LN2_B], TK};
    CK(launch_ln_fwd(s0, s1, H, st), "layernorm fwd");
  }
  // FFN first layers (ReLU + dropout fused), fusion_model.py:53-65
  set_drop(g.nt(w.Y, H, P[CAMO_P_F1_W0], H, P[CAMO_P_F1_B0], w.H1, 2 * H, T, 2 * H, H, GF_RELU), SITE_FFN_RG);
  set_drop(g.nt(w.Y2, H, P[CAMO_P_F2_W0], H, P[CAMO_P_F2_B0], w.H2, 2 * H, TK, 2 * H, H, GF_RELU), SITE_FFN_KG);
  CK(g.run(), "ffn layer 0");
  // per-sample means of Y and H1d (the other schedules' kernels accumulate them as they produce the pooled tensors)
  SegMean sm[4] = {{w.Y, H, H, rg_offsets, 0, w.Ymean, H}, {w.H1, 2 * H, 2 * H, rg_offsets, 0, w.H1mean, 2 * H},
                   {w.Y2, H, H, nullptr, Nk, w.Y2mean, H}, {w.H2, 2 * H, 2 * H, nullptr, Nk, w.H2mean, 2 * H}};
  CK(launch_seg_mean(sm, 4, B, max_nr > Nk ? max_nr : Nk, st), "pool");
  return 0;
}

// the per-sample tail as fp32 GEMM launches: the second FFN layer on the means (mean-pool linearity), the fusion layer, the heads
int forward_tail_gemms(const Batch& x, float* outs, const FusedLoss* fl) {
  const float* const* P = x.P; const Ws& w = x.w;
  const int H = x.dims->hidden_dim, B = x.B;
  GB gt = tail_gemms(x);
  set_res(gt.nt(w.H1mean, 2 * H, P[CAMO_P_F1_W3], 2 * H, P[CAMO_P_F1_B3], w.comb, 2 * H, B, H, 2 * H), w.Ymean, H);
  set_res(gt.nt(w.H2mean, 2 * H, P[CAMO_P_F2_W3], 2 * H, P[CAMO_P_F2_B3], w.comb + H, 2 * H, B, H, 2 * H), w.Y2mean, H);
  CK(gt.run(), "ffn layer 3 on pooled rows");
  // fusion layer (fusion_model.py:68-73,138-139)
  set_drop(gt.nt(w.comb, 2 * H, P[CAMO_P_FU_W0], 2 * H, P[CAMO_P_FU_B0], w.F1, H, B, H, 2 * H, GF_RELU), SITE_FUSE);
  CK(gt.run(), "fusion layer 0");
  gt.nt(w.F1, H, P[CAMO_P_FU_W3], H, P[CAMO_P_FU_B3], w.fused, H, B, H, H);
  CK(gt.run(), "fusion layer 3");
  return heads_forward(x, CAMO_P_HEADS, H, outs, fl);
}

// fl: the training call's labels, for the launch that camo_plan_t::loss names (null: no loss in this forward)
int forward_impl(Call& c, const Batch& x, float* outs, float* attn_rg2kg, float* attn_kg2rg, const FusedLoss* fl) {
  const camo_dims_t& d = *x.dims;
  if (x.plan.nodes == CAMO_NODES_LATE) return forward_late(x, outs, fl);
  if (!x.P[CAMO_P_RG_PROJ_W] && d.rg_dim != d.hidden_dim) return fail(CAMO_E_ARG, "rg_proj weight missing but rg_dim != hidden_dim");
  if (!x.P[CAMO_P_KG_PROJ_W] && d.kg_dim != d.hidden_dim) return fail(CAMO_E_ARG, "kg_proj weight missing but kg_dim != hidden_dim");
  if (x.plan.nodes == CAMO_NODES_FUSED) {
    if (int e = forward_nodes17(c, x, attn_rg2kg, attn_kg2rg)) return e;
    if (x.plan.tail >= CAMO_TAIL_PLANES) return tail_planes_forward(x, outs, fl);
    if (x.plan.tail == CAMO_TAIL_ONE_LAUNCH) return tail17(c, x, outs, fl);
  } else if (x.plan.nodes == CAMO_NODES_BF16) {
    if (int e = forward_nodes16(x, attn_rg2kg, attn_kg2rg)) return e;
  } else {
    if (int e = forward_nodes_general(x, attn_rg2kg, attn_kg2rg)) return e;
  }
  return forward_tail_gemms(x, outs, fl);
}

// the per-sample tail's backward as fp32 GEMM launches: heads, fusion layer, pooled second FFN layer
int backward_tail_gemms(const Batch& x, const float* outs, const float* d_outs, int pre_activation, bool heads_out_done) {
  const float* const* P = x.P; float* const* Gr = x.Gr; const Ws& w = x.w; const DropCfg& drop = x.drop;
  const int H = x.dims->hidden_dim, B = x.B;
  if (int e = heads_backward(x, CAMO_P_HEADS, H, outs, d_outs, pre_activation, heads_out_done)) return e;
  GB gt = tail_gemms(x);
  // fusion layer
  set_relu_bwd(gt.nn(w.dfused, H, P[CAMO_P_FU_W3], H, w.dF1, H, B, H, H), w.F1, H, drop.scale);
  gt.tn(w.dfused, H, w.F1, H, Gr[CAMO_P_FU_W3], H, Gr[CAMO_P_FU_B3], H, H, B);
  CK(gt.run(), "fusion layer 3 bwd");
  gt.nn(w.dF1, H, P[CAMO_P_FU_W0], 2 * H, w.dcomb, 2 * H, B, 2 * H, H);
  gt.tn(w.dF1, H, w.comb, 2 * H, Gr[CAMO_P_FU_W0], 2 * H, Gr[CAMO_P_FU_B0], H, 2 * H, B);
  CK(gt.run(), "fusion layer 0 bwd");
  // pooled second FFN layer: d(mean H1d) = dpool.W2 ; dW2 += dpool^T.mean(H1d) ; db2 += sum_b dpool
  gt.nn(w.dcomb, 2 * H, P[CAMO_P_F1_W3], 2 * H, w.dHm1, 2 * H, B, 2 * H, H);
  gt.nn(w.dcomb + H, 2 * H, P[CAMO_P_F2_W3], 2 * H, w.dHm2, 2 * H, B, 2 * H, H);
  gt.tn(w.dcomb, 2 * H, w.H1mean, 2 * H, Gr[CAMO_P_F1_W3], 2 * H, Gr[CAMO_P_F1_B3], H, 2 * H, B);
  gt.tn(w.dcomb + H, 2 * H, w.H2mean, 2 * H, Gr[CAMO_P_F2_W3], 2 * H, Gr[CAMO_P_F2_B3], H, 2 * H, B);
  CK(gt.run(), "ffn layer 3 bwd (pooled)");
  return 0;
}

// ---- node-level backward of the general schedule
int backward_nodes_general(const Batch& x) {
  const camo_dims_t& d = *x.dims; const float* const* P = x.P; float* const* Gr = x.Gr; const Ws& w = x.w; const DropCfg& drop = x.drop; hipStream_t st = x.st;
  const float* rg = x.rg; const float* kg = x.kg; const int32_t* rg_offsets = x.rg_offsets; const int32_t* row_sample = x.bd.row_sample; const float* inv_nr = x.bd.inv_nr;
  const int H = d.hidden_dim, D = d.rg_dim, Dk = d.kg_dim, B = x.B, T = x.T, Nk = x.Nk, TK = B * Nk, nh = d.num_heads, max_nr = x.max_nr;
  const bool has_rgp = P[CAMO_P_RG_PROJ_W] != nullptr, has_kgp = P[CAMO_P_KG_PROJ_W] != nullptr;
  const float* R = has_rgp ? w.R : rg;
  const float* G = has_kgp ? w.G : kg;
  GB g(drop, x.precision, st);
  {
    BcastSeg s0{w.H1, w.dHm1, 2 * H, row_sample, inv_nr, 0, w.dH1, T};
    BcastSeg s1{w.H2, w.dHm2, 2 * H, nullptr, nullptr, Nk, w.dH2, TK};
    CK(launch_relu_bcast_bwd(s0, s1, 2 * H, drop.scale, st), "relu bcast bwd");
  }
  // first FFN layer: dY = bcast(dpool)/n + dH1.W1 ; dW1 += dH1^T.Y
  set_bcast(g.nn(w.dH1, 2 * H, P[CAMO_P_F1_W0], H, w.dY, H, T, H, 2 * H), w.dcomb, 2 * H, row_sample, inv_nr, 0);
  set_bcast(g.nn(w.dH2, 2 * H, P[CAMO_P_F2_W0], H, w.dY2, H, TK, H, 2 * H), w.dcomb + H, 2 * H, nullptr, nullptr, Nk);
  g.tn(w.dH1, 2 * H, w.Y, H, Gr[CAMO_P_F1_W0], H, Gr[CAMO_P_F1_B0], 2 * H, H, T);
  g.tn(w.dH2, 2 * H, w.Y2, H, Gr[CAMO_P_F2_W0], H, Gr[CAMO_P_F2_B0], 2 * H, H, TK);
  CK(g.run(), "ffn layer 0 bwd");
  {
    LnBwdSeg s0{w.U, w.dY, w.st1, P[CAMO_P_LN1_W], w.dU, Gr[CAMO_P_LN1_W], Gr[CAMO_P_LN1_B], T};
    LnBwdSeg s1{w.U2, w.dY2, w.st2, P[CAMO_P_LN2_W], w.dU2, Gr[CAMO_P_LN2_W], Gr[CAMO_P_LN2_B], TK};
    CK(launch_ln_bwd(s0, s1, H, st), "layernorm bwd");
  }
  // out-projections
  g.nn(w.dU, H, P[CAMO_P_A1_OUT_W], H, w.dO, H, T, H, H);
  g.nn(w.dU2, H, P[CAMO_P_A2_OUT_W], H, w.dO2, H, TK, H, H);
  g.tn(w.dU, H, w.O, H, Gr[CAMO_P_A1_OUT_W], H, Gr[CAMO_P_A1_OUT_B], H, H, T);
  g.tn(w.dU2, H, w.O2, H, Gr[CAMO_P_A2_OUT_W], H, Gr[CAMO_P_A2_OUT_B], H, H, TK);
  CK(g.run(), "out-projection bwd");
  CK(launch_attn_rg2kg_bwd(w.Q, w.KV, w.P, w.dO, rg_offsets, w.dQ, w.dKV, B, max_nr, H, nh, Nk, drop, st), "attn rg2kg bwd");
  CK(launch_attn_kg2rg_bwd(w.Q2, w.KV2, w.P2, w.dO2, w.O2, rg_offsets, w.dQ2, w.dKV2, w.dS2, B, max_nr, H, nh, Nk, drop, st), "attn kg2rg bwd");
  // in-projection weight gradients, and the gradients flowing into R and G
  const size_t HH = (size_t)H * H;
  g.tn(w.dQ, H, R, H, Gr[CAMO_P_A1_IN_W], H, Gr[CAMO_P_A1_IN_B], H, H, T);
  g.tn(w.dKV2, 2 * H, R, H, Gr[CAMO_P_A2_IN_W] + HH, H, Gr[CAMO_P_A2_IN_B] + H, 2 * H, H, T);
  g.tn(w.dKV, 2 * H, G, H, Gr[CAMO_P_A1_IN_W] + HH, H, Gr[CAMO_P_A1_IN_B] + H, 2 * H, H, TK);
  g.tn(w.dQ2, H, G, H, Gr[CAMO_P_A2_IN_W], H, Gr[CAMO_P_A2_IN_B], H, H, TK);
  if (has_rgp) set_res(g.nn(w.dQ, H, P[CAMO_P_A1_IN_W], H, w.dR, H, T, H, H), w.dU, H);
  if (has_kgp) set_res(g.nn(w.dQ2, H, P[CAMO_P_A2_IN_W], H, w.dG, H, TK, H, H), w.dU2, H);
  CK(g.run(), "in-projection bwd");
  if (has_rgp) set_res(g.nn(w.dKV2, 2 * H, P[CAMO_P_A2_IN_W] + HH, H, w.dR, H, T, H, 2 * H), w.dR, H);
  if (has_kgp) set_res(g.nn(w.dKV, 2 * H, P[CAMO_P_A1_IN_W] + HH, H, w.dG, H, TK, H, 2 * H), w.dG, H);
  CK(g.run(), "k|v input gradients");
  if (has_rgp) g.tn(w.dR, H, rg, D, Gr[CAMO_P_RG_PROJ_W], D, Gr[CAMO_P_RG_PROJ_B], H, D, T);
  if (has_kgp) g.tn(w.dG, H, kg, Dk, Gr[CAMO_P_KG_PROJ_W], Dk, Gr[CAMO_P_KG_PROJ_B], H, Dk, TK);
  CK(g.run(), "input projection bwd");
  return 0;
}

int backward_impl(Call& c, const Batch& x, const float* outs, const float* d_outs, int pre_activation, bool heads_out_done) {
  if (x.plan.nodes == CAMO_NODES_LATE) return backward_late(x, outs, d_outs, pre_activation, heads_out_done);
  if (x.plan.tail == CAMO_TAIL_PLANES_TRAIN) { if (int e = tail_planes_backward(x)) return e; }
  else if (int e = backward_tail_gemms(x, outs, d_outs, pre_activation, heads_out_done)) return e;
  if (x.plan.tail_event == CAMO_EVENT_BEFORE_NODES) CK(record_tail_event(c, x.st), "tail event");
  if (x.plan.nodes == CAMO_NODES_FUSED) return backward_nodes17(c, x);
  if (x.plan.nodes == CAMO_NODES_BF16) return backward_nodes16(x);
  return backward_nodes_general(x);
}

}  // namespace

extern "C" {

int camo_abi_version(void) { return CAMO_ABI_VERSION; }
const char* camo_last_error(void) { return g_err.c_str(); }

size_t camo_workspace_bytes(const camo_dims_t* dims, int32_t B, int32_t T, int32_t Nk) {
  if (check_dims(dims, B, T, Nk)) return 0;
  return carve(*dims, B, T, Nk, nullptr).bytes;
}

size_t camo_batch_desc_bytes(int32_t B, int32_t T) {
  if (B < 1 || T < B) { fail(CAMO_E_ARG, "need B >= 1 and T >= B"); return 0; }
  return desc_carve(B, T, nullptr).bytes;
}

int camo_prepare_batch(const int32_t* rg_offsets, int32_t B, int32_t T, int32_t max_nr, void* desc, size_t desc_bytes, void* stream) {
  if (!rg_offsets || !desc || B < 1 || T < B || max_nr < 1 || max_nr > T) return fail(CAMO_E_ARG, "bad prepare_batch arguments");
  const Desc d = desc_carve(B, T, desc);
  if (desc_bytes < d.bytes) return fail(CAMO_E_WORKSPACE, "descriptor buffer smaller than camo_batch_desc_bytes()");
  CK(launch_rowmap(rg_offsets, d.row_sample, d.inv_nr, d.tile_off, d.tile_desc, B, T / 32 + B, max_nr, static_cast<hipStream_t>(stream)), "rowmap");
  return 0;
}

int camo_gather_batch(const float* rg_all, const int64_t* sample_offsets, const float* kg_all, const int64_t* y_all, const float* e_all, const float* s_all,
                      const int64_t* idx, int32_t B, int32_t T, int32_t rg_dim, int32_t kg_floats, float* rg_out, float* kg_out, int32_t* offsets_out,
                      int64_t* y_out, float* e_out, float* s_out, float noise_std, uint64_t seed, void* stream) {
  if (!rg_all || !sample_offsets || !kg_all || !y_all || !e_all || !s_all || !idx || !rg_out || !kg_out || !offsets_out || !y_out || !e_out || !s_out)
    return fail(CAMO_E_ARG, "null pointer argument");
  if (B < 1 || T < B) return fail(CAMO_E_ARG, "need B >= 1 and T >= B");
  if (B > 4096 || rg_dim < 4 || (rg_dim & 3) || rg_dim > 1024 || kg_floats < 2 || (kg_floats & 1) || noise_std < 0.f)
    return fail(CAMO_E_UNSUPPORTED, "camo_gather_batch: B <= 4096, rg_dim a multiple of 4 (<= 1024), an even number of KG floats per sample");
  CK(launch_gather_batch(rg_all, reinterpret_cast<const long long*>(sample_offsets), kg_all, reinterpret_cast<const long long*>(y_all), e_all, s_all,
                         reinterpret_cast<const long long*>(idx), B, T, rg_dim, kg_floats, rg_out, kg_out, offsets_out, reinterpret_cast<long long*>(y_out),
                         e_out, s_out, noise_std, seed, static_cast<hipStream_t>(stream)), "gather batch");
  return 0;
}

int camo_forward(const camo_dims_t* dims, const float* const* params, const float* rg, const int32_t* rg_offsets,
                 const void* batch_desc,
                 const float* kg, int32_t B, int32_t T, int32_t Nk, int32_t max_nr, void* workspace,
                 size_t workspace_bytes, float* outs, float* attn_rg2kg, float* attn_kg2rg, int32_t training,
                 uint64_t seed, int32_t precision, int32_t flags, void* stream) {
  return camo_forward_cached(dims, params, rg, rg_offsets, batch_desc, kg, B, T, Nk, max_nr, workspace, workspace_bytes, outs, attn_rg2kg, attn_kg2rg,
                             training, seed, precision, flags, nullptr, 0, nullptr, stream);
}

int camo_forward_cached(const camo_dims_t* dims, const float* const* params, const float* rg, const int32_t* rg_offsets,
                        const void* batch_desc, const float* kg, int32_t B, int32_t T, int32_t Nk, int32_t max_nr, void* workspace,
                        size_t workspace_bytes, float* outs, float* attn_rg2kg, float* attn_kg2rg, int32_t training,
                        uint64_t seed, int32_t precision, int32_t flags, void* shadows, int32_t shadows_valid, int32_t* shadows_state,
                        void* stream) {
  Call c;
  if (shadows_state) *shadows_state = 0;
  if (shadows_valid && !shadows) return fail(CAMO_E_ARG, "shadows_valid without a shadow buffer");
  // A call that saves for camo_backward would leave the backward's transposed shadows in the caller's buffer, where camo_backward
  // (which takes no shadow argument) cannot find them, and the clears it defers to the first backward kernel would end with this
  // call: the training pair is camo_forward_loss_backward, which owns both halves.
  if (shadows && !(flags & CAMO_FWD_INFERENCE))
    return fail(CAMO_E_UNSUPPORTED, "camo_forward_cached with a shadow buffer serves inference calls only (flags must contain CAMO_FWD_INFERENCE)");
  if (shadows && (reinterpret_cast<uintptr_t>(shadows) & 255)) return fail(CAMO_E_ARG, "the shadow buffer must be 256-byte aligned");
  if (int e = check_dims(dims, B, T, Nk)) return e;
  // (training mode with dropout: the reference's maps are the probabilities after attention dropout -- today's schedules model that)
  if (training && dims->dropout > 0.f) flags &= ~CAMO_FWD_FUSED_MAPS;
  Batch x{dims, params, nullptr, rg, rg_offsets, batch_desc, kg, B, T, Nk, max_nr, workspace, workspace_bytes, training, seed, precision, static_cast<hipStream_t>(stream)};
  plan_batch(x, (flags & CAMO_FWD_INFERENCE) ? CALL_INFERENCE : CALL_FORWARD_SAVE, attn_rg2kg || attn_kg2rg || (flags & CAMO_FLAG_ATTN_MAPS),
             (attn_rg2kg || attn_kg2rg) && (flags & CAMO_FWD_FUSED_MAPS) != 0);
  // (a call that takes a schedule without shadows leaves the caller's buffer alone: a promise is then simply not used)
  if (x.plan.shadows) { c.shadows = shadows; c.shadows_valid = shadows && shadows_valid != 0; c.fold_missing = shadows && shadows_valid == 2; }
  if (int e = open_batch(x, c, outs != nullptr)) return e;
  c.tail_skip = x.opt->tail_skip_arrival;
  const int rc = forward_impl(c, x, outs, attn_rg2kg, attn_kg2rg, nullptr);
  if (c.tail_skip_taken) dims->options->tail_skip_arrival = 0;
  if (rc == 0 && shadows_state) *shadows_state = c.shadows_state;
  return rc;
}

int camo_backward(const camo_dims_t* dims, const float* const* params, float* const* grads, const float* rg,
                  const int32_t* rg_offsets, const void* batch_desc, const float* kg, int32_t B,
                  int32_t T, int32_t Nk, int32_t max_nr, void* workspace, size_t workspace_bytes, const float* outs,
                  const float* d_outs, int32_t d_outs_pre_activation, int32_t training, uint64_t seed, int32_t precision,
                  int32_t flags, void* stream) {
  Call c;
  if (int e = check_dims(dims, B, T, Nk)) return e;
  Batch x{dims, params, grads, rg, rg_offsets, batch_desc, kg, B, T, Nk, max_nr, workspace, workspace_bytes, training, seed, precision, static_cast<hipStream_t>(stream)};
  plan_batch(x, CALL_BACKWARD, (flags & CAMO_FLAG_ATTN_MAPS) != 0);
  if (int e = open_batch(x, c, grads && outs && d_outs)) return e;
  return backward_impl(c, x, outs, d_outs, d_outs_pre_activation, false);
}

int camo_forward_loss_backward(const camo_dims_t* dims, const float* const* params, float* const* grads, const float* rg,
                               const int32_t* rg_offsets, const void* batch_desc, const float* kg,
                               int32_t B, int32_t T, int32_t Nk, int32_t max_nr, void* workspace, size_t workspace_bytes,
                               const int64_t* y, const float* e, const float* s, float* outs, float* loss_terms, int32_t* pred,
                               int32_t training, uint64_t seed, int32_t precision, void* tail_event, void* shadows,
                               int32_t shadows_valid, void* stream) {
  Call c;
  if (!dims || !grads || !y || !e || !s || !outs || !loss_terms) return fail(CAMO_E_ARG, "null pointer argument");
  if (shadows_valid && !shadows) return fail(CAMO_E_ARG, "shadows_valid without a shadow buffer");
  if (int rc = check_dims(dims, B, T, Nk)) return rc;
  Batch x{dims, params, grads, rg, rg_offsets, batch_desc, kg, B, T, Nk, max_nr, workspace, workspace_bytes, training, seed, precision, static_cast<hipStream_t>(stream)};
  plan_batch(x, CALL_TRAIN, false);
  // external shadows are used by the fused schedule only; whether the call takes it is known from its arguments
  // (a call that takes another schedule -- Nk > 16, a 5000-node sample, ... -- builds what it needs in its workspace and leaves the
  // external shadows alone: the promise is simply not used)
  if (shadows && x.plan.shadows) {
    if (reinterpret_cast<uintptr_t>(shadows) & 255) return fail(CAMO_E_ARG, "the shadow buffer must be 256-byte aligned");
    c.shadows = shadows; c.shadows_valid = shadows_valid != 0;
  }
  if (int rc = open_batch(x, c, true)) return rc;
  c.tail_event = static_cast<hipEvent_t>(tail_event);
  c.tail_skip = x.opt->tail_skip_arrival;
  const camo_plan_t& pl = x.plan;
  const FusedLoss fl{y, e, s, loss_terms, pred};
  int rc = forward_impl(c, x, outs, nullptr, nullptr, pl.loss == CAMO_LOSS_LAUNCH ? nullptr : &fl);
  if (c.tail_skip_taken) dims->options->tail_skip_arrival = 0;
  if (rc) return rc;
  if (pl.loss == CAMO_LOSS_TAIL) {
    // fused schedule + one-launch tail: node-level forward, [tail forward + loss + tail backward], node-level backward
    if (pl.tail_event == CAMO_EVENT_BEFORE_NODES) CK(record_tail_event(c, x.st), "tail event");
    rc = backward_nodes17(c, x);
  } else if (pl.loss == CAMO_LOSS_HEADS) {
    rc = backward_impl(c, x, outs, nullptr, 1, true);
  } else {
    // large batches / many classes: the three steps as separate launches, d(loss)/d(pre-activation) staged in the workspace
    CK(launch_loss(outs, reinterpret_cast<const long long*>(y), e, s, B, dims->num_classes, loss_terms, nullptr, x.w.dlog, pred, x.st), "loss");
    rc = backward_impl(c, x, outs, x.w.dlog, 1, false);
  }
  if (rc == 0 && pl.tail_event == CAMO_EVENT_END) CK(record_tail_event(c, x.st), "tail event");   // (schedules without an early point)
  return rc;
}

int camo_loss(const float* outs, const int64_t* y, const float* e, const float* s, int32_t B, int32_t num_classes,
              float* loss_terms, float* d_outs, float* d_pre, int32_t* pred, void* stream) {
  if (!outs || !y || !e || !s || !loss_terms) return fail(CAMO_E_ARG, "null pointer argument");
  if (B < 1 || num_classes < 1 || num_classes > 64) return fail(CAMO_E_ARG, "need B >= 1 and 1 <= num_classes <= 64");
  CK(launch_loss(outs, reinterpret_cast<const long long*>(y), e, s, B, num_classes, loss_terms, d_outs, d_pre, pred,
                 static_cast<hipStream_t>(stream)), "loss");
  return 0;
}

int camo_grad_sumsq(const float* g, size_t n, float* sumsq, void* stream) {
  if (!g || !sumsq || n == 0) return fail(CAMO_E_ARG, "null pointer or empty buffer");
  CK(launch_sumsq(g, n, sumsq, static_cast<hipStream_t>(stream)), "grad sumsq");
  return 0;
}

size_t camo_shadow_bytes(const camo_dims_t* dims) {
  if (!dims || !fused17_dims(*dims)) return 0;
  return shadow_carve(nullptr).bytes;
}

int camo_clip_adamw_shadows(const camo_dims_t* dims, const float* const* params, float* p, float* g, float* m, float* v, size_t n,
                            float* sumsq, float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay,
                            int32_t step, int32_t zero_grads, void* shadows, void* stream) {
  if (!dims || !params || !p || !g || !m || !v || !sumsq || !shadows || n == 0) return fail(CAMO_E_ARG, "null pointer or empty buffer");
  if (step < 1) return fail(CAMO_E_ARG, "step is 1-based");
  if (!fused17_dims(*dims)) return fail(CAMO_E_UNSUPPORTED, "weight shadows exist for the fused schedule's configuration only");
  if (reinterpret_cast<uintptr_t>(shadows) & 255) return fail(CAMO_E_ARG, "the shadow buffer must be 256-byte aligned");
  const ShadowSet x = shadow_carve(shadows);
  AdamShadowArgs a; std::memset(&a, 0, sizeof(a));
  struct Cov { size_t off, len; } cov[ADAM_SHADOW_MAXB];
  int ncov = 0;
  bool ok = true;
  for (const ShadowSlice& sl : k_shadow_slices) {      // one block per slice: the update leaves its rows in the shadows the forward reads them from
    const float* src = params[sl.param] ? params[sl.param] + (size_t)sl.r0 * sl.cols : nullptr;
    if (!src || src < p || src + (size_t)sl.rows * sl.cols > p + n) { ok = false; break; }
    AdamShadowBlock& B = a.blk[a.nblk++];
    B.off = (size_t)(src - p); B.rows = sl.rows; B.cols = sl.cols; B.plain = x.*sl.plain; B.pN = sl.pN; B.pn0 = sl.pn0;
    B.trans = sl.trans ? x.*sl.trans : nullptr; B.tK = sl.tK; B.tk0 = sl.tk0;
    cov[ncov++] = Cov{B.off, (size_t)sl.rows * sl.cols};
  }
  if (!ok) return fail(CAMO_E_ARG, "the shadowed parameters must lie inside the flat buffer [p, p + n)");
  // the rest of the flat buffer: the gaps between the shadowed blocks, in address order
  for (int i = 1; i < ncov; ++i)
    for (int j = i; j > 0 && cov[j].off < cov[j - 1].off; --j) { const Cov t = cov[j]; cov[j] = cov[j - 1]; cov[j - 1] = t; }
  size_t at = 0;
  for (int i = 0; i <= ncov; ++i) {
    const size_t end = i < ncov ? cov[i].off : n;
    if (end < at) return fail(CAMO_E_ARG, "overlapping parameter blocks");
    if (end > at) {
      if (a.nrange >= ADAM_SHADOW_MAXR) return fail(CAMO_E_ARG, "too many gaps between the shadowed parameters");
      if ((at & 3) || ((end - at) & 3)) return fail(CAMO_E_ARG, "parameters must be 16-byte aligned slices of the flat buffer");
      a.range_begin[a.nrange] = at; a.range_len[a.nrange++] = end - at;
    }
    if (i < ncov) at = cov[i].off + cov[i].len;
  }
  CK(launch_clip_adamw_shadows(p, g, m, v, sumsq, max_norm, lr, beta1, beta2, eps, weight_decay, step, zero_grads, a,
                               static_cast<hipStream_t>(stream)), "clip+adamw+shadows");
  return 0;
}

int camo_clip_adamw(float* p, float* g, float* m, float* v, size_t n, float* sumsq, float max_norm, float lr,
                    float beta1, float beta2, float eps, float weight_decay, int32_t step, int32_t zero_grads, void* stream) {
  if (!p || !g || !m || !v || !sumsq || n == 0) return fail(CAMO_E_ARG, "null pointer or empty buffer");
  if (step < 1) return fail(CAMO_E_ARG, "step is 1-based");
  CK(launch_clip_adamw(p, g, m, v, n, sumsq, max_norm, lr, beta1, beta2, eps, weight_decay, step, zero_grads,
                       static_cast<hipStream_t>(stream)), "clip+adamw");
  return 0;
}

int camo_debug_gemm(const float* A, int32_t lda, const float* B, int32_t ldb, float* C, int32_t ldc, const float* bias,
                    const float* res, int32_t ldr, float* bias_grad, int32_t M, int32_t N, int32_t K, int32_t flags,
                    int32_t precision, void* stream) {
  if (!A || !B || !C || M < 1 || N < 1 || K < 1) return fail(CAMO_E_ARG, "bad gemm arguments");
  GB g(make_drop(0, 0.f, 0), precision, static_cast<hipStream_t>(stream));
  GemmProb& p = g.add(A, lda, B, ldb, C, ldc, M, N, K, flags);
  p.bias = bias; p.res = res; p.ldr = ldr; p.bias_grad = bias_grad;
  CK(g.run(), "debug gemm");
  return 0;
}

int camo_debug_gemm_batch(const void* const* ptrs, const int32_t* ints, const float* aux_scale, int32_t n, int32_t precision,
                          float drop_p, uint64_t seed, void* stream) {
  if (!ptrs || !ints || !aux_scale || n < 1 || n > GEMM_MAXP) return fail(CAMO_E_ARG, "bad gemm batch arguments");
  GB g(make_drop(1, drop_p, seed), precision, static_cast<hipStream_t>(stream));
  for (int i = 0; i < n; ++i) {
    const void* const* q = ptrs + 8 * i;
    const int32_t* v = ints + 10 * i;
    if (!q[0] || !q[1] || !q[2] || v[0] < 1 || v[1] < 1 || v[2] < 1) return fail(CAMO_E_ARG, "bad gemm batch problem");
    GemmProb& p = g.add(static_cast<const float*>(q[0]), v[3], static_cast<const float*>(q[1]), v[4],
                        static_cast<float*>(const_cast<void*>(q[2])), v[5], v[0], v[1], v[2], v[7]);
    p.bias = static_cast<const float*>(q[3]); p.res = static_cast<const float*>(q[4]); p.ldr = v[6];
    p.bias_grad = static_cast<float*>(const_cast<void*>(q[5]));
    p.row_sample = static_cast<const int*>(q[6]); p.inv_nr = static_cast<const float*>(q[7]);
    p.drop_site = (uint32_t)v[8]; p.uniform_n = v[9]; p.aux_scale = aux_scale[i];
  }
  CK(g.run(), "debug gemm batch (a refused combination: csrc/gemm.h)");
  return 0;
}

int camo_debug_gemm16(const void* A16, int32_t lda, const void* B16, int32_t ldb, float* C, int32_t ldc, void* C16,
                      int32_t ldc16, const float* bias, const float* res, int32_t ldr, float* bias_grad, int32_t M,
                      int32_t N, int32_t K, int32_t flags, void* stream) {
  if (!A16 || !B16 || (!C && !C16) || M < 1 || N < 1 || K < 1) return fail(CAMO_E_ARG, "bad gemm16 arguments");
  Gemm16Batch gb;
  std::memset(&gb, 0, sizeof(gb));
  gb.drop = make_drop(0, 0.f, 0);
  Gemm16Prob& p = gb.p[0];
  gb.n = 1;
  p.A = static_cast<const unsigned short*>(A16); p.lda = lda; p.B = static_cast<const unsigned short*>(B16); p.ldb = ldb;
  p.C = C; p.ldc = ldc; p.C16 = static_cast<unsigned short*>(C16); p.ldc16 = ldc16;
  p.bias = bias; p.res = res; p.ldr = ldr; p.bias_grad = bias_grad; p.M = M; p.N = N; p.K = K; p.flags = flags; p.aux_scale = 1.f;
  CK(launch_gemm16_batch(gb, Gemm16Knobs{}, static_cast<hipStream_t>(stream)), "debug gemm16");
  return 0;
}

int camo_options_init(camo_options_t* o) {
  if (!o) return fail(CAMO_E_ARG, "options is null");
  *o = k_default_options;
  return 0;
}

int camo_options_set(camo_options_t* o, const char* name, int32_t value) {
  if (!o || !name) return fail(CAMO_E_ARG, "options or option name is null");
  struct Field { const char* name; int32_t camo_options_t::*m; };
  static const Field fields[] = {
      {"sched16", &camo_options_t::sched16}, {"fused", &camo_options_t::fused}, {"tail17", &camo_options_t::tail17}, {"fused_rt", &camo_options_t::fused_rt},
      {"wide2", &camo_options_t::wide2}, {"fused_one", &camo_options_t::fused_one}, {"wide_front_rt", &camo_options_t::wide_front_rt}, {"tailw", &camo_options_t::tailw},
      {"tailw_bwd", &camo_options_t::tailw_bwd}, {"param_space", &camo_options_t::param_space}, {"tn_big", &camo_options_t::tn_big},
      {"fused_variant", &camo_options_t::fused_variant}, {"back_lead", &camo_options_t::back_lead}, {"tn_balance", &camo_options_t::tn_balance},
      {"tn_kcap", &camo_options_t::tn_kcap}, {"tn_exp", &camo_options_t::tn_exp}, {"exp", &camo_options_t::exp}, {"fused_save", &camo_options_t::fused_save},
      {"tail_skip_arrival", &camo_options_t::tail_skip_arrival}, {"wide2_bwd", &camo_options_t::wide2_bwd}};
  for (const Field& f : fields)
    if (std::strcmp(name, f.name) == 0) { o->*(f.m) = value; return 0; }
  return fail(CAMO_E_ARG, std::string("unknown option ") + name);
}

int camo_debug_set_stamps(void* buf, int32_t blocks_per_kernel) {
  g_dbg_stamps = static_cast<unsigned long long*>(buf); g_dbg_stamp_blocks = blocks_per_kernel;
  return 0;
}

int camo_prof_begin(int32_t max_launches) {
  CK(gemm_prof_begin(max_launches), "prof begin");
  return 0;
}

int camo_tail_timeouts(uint32_t* count) {
  if (!count) return fail(CAMO_E_ARG, "null pointer argument");
  unsigned int n = 0;
  CK(tail_timeouts(&n), "tail timeouts");
  *count = n;
  return 0;
}

int camo_tail_poison_to_grads(float* flat_grads, void* stream) {
  if (!flat_grads) return fail(CAMO_E_ARG, "camo_tail_poison_to_grads: null gradient buffer");
  const int e = launch_tail_poison_to_grads(flat_grads, static_cast<hipStream_t>(stream));
  return e ? fail_hip(e, "camo_tail_poison_to_grads") : 0;
}

int camo_prof_kind(int32_t kind, double* ms, int32_t* launches, double* flops) {
  int n = 0;
  CK(gemm_prof_kind(kind, ms, &n, flops), "prof kind");
  if (launches) *launches = n;
  return 0;
}

int camo_prof_end(double* gemm_ms, int32_t* gemm_launches, double* gemm_flops) {
  int n = 0;
  CK(gemm_prof_end(gemm_ms, &n, gemm_flops), "prof end");
  if (gemm_launches) *gemm_launches = n;
  return 0;
}

int64_t camo_debug_ws_offset(const camo_dims_t* dims, int32_t B, int32_t T, int32_t Nk, const char* name) {
  if (check_dims(dims, B, T, Nk) || !name) return -1;
  return ws_offset_of(*dims, B, T, Nk, name);
}

int camo_debug_plan(const camo_dims_t* dims, int32_t has_projections, int32_t B, int32_t T, int32_t Nk, int32_t max_nr,
                    int32_t precision, int32_t flags, int32_t call_kind, int32_t cus, camo_plan_t* out) {
  if (int e = check_dims(dims, B, T, Nk)) return e;
  if (!out) return fail(CAMO_E_ARG, "null pointer argument");
  if (max_nr < 1 || max_nr > T) return fail(CAMO_E_ARG, "max_nr out of range");
  if (precision != CAMO_PREC_F32 && precision != CAMO_PREC_BF16) return fail(CAMO_E_ARG, "unknown precision");
  if (call_kind != CAMO_CALL_FORWARD && call_kind != CAMO_CALL_BACKWARD && call_kind != CAMO_CALL_TRAIN) return fail(CAMO_E_ARG, "unknown call kind");
  const CallKind kind = call_kind == CAMO_CALL_TRAIN ? CALL_TRAIN : (call_kind == CAMO_CALL_BACKWARD ? CALL_BACKWARD : ((flags & CAMO_FWD_INFERENCE) ? CALL_INFERENCE : CALL_FORWARD_SAVE));
  *out = make_plan(PlanIn{options_of(dims), *dims, (has_projections & 1) != 0, (has_projections & 2) != 0, precision, B, T, Nk, max_nr, kind,
                          kind != CALL_TRAIN && (flags & CAMO_FLAG_ATTN_MAPS) != 0, (flags & CAMO_FWD_FUSED_MAPS) != 0, cus < 0 ? device_cus() : cus});
  return 0;
}

}  // extern "C"
