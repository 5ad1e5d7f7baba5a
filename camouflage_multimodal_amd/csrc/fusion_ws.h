// The buffers the fusion model runs on, each stated once: the batch descriptor, the per-call workspace, the caller-owned weight
// shadows, and which parameter rows every weight shadow holds.  Host only; included by fusion_abi.hip alone, whose launch sequences
// read these structs and compute no offset themselves.
#pragma once
#include <cstring>

#include "../../include/camo_fusion.h"
#include "abi_util.h"
#include "fused_rows.h"

namespace camo_ws {
using camo_abi::Carver;

// How carve() hands out a buffer: c(field, elements[, name]).  Take only assigns addresses: the call path, on which a name is an unused
// argument.  Find also remembers the buffer that carries one name (camo_debug_ws_offset), so a name is resolved by the code that carves it.
struct Take : Carver {
  using Carver::Carver;
  template <typename T> void operator()(T*& p, size_t n, const char* = nullptr) { p = take<T>(n); }
  void name(const void*, const char*) {}
};
struct Find : Carver {
  const char* want; const void* hit = nullptr;
  Find(void* base, const char* w) : Carver(base), want(w) {}
  template <typename T> void operator()(T*& p, size_t n, const char* nm = nullptr) { p = take<T>(n); name(p, nm); }
  void name(const void* p, const char* nm) { if (nm && std::strcmp(nm, want) == 0) hit = p; }
};
// consecutive members of one taken block, in 4-byte words (every length a multiple of 4 words keeps them 16-byte aligned)
template <class C> struct Members {
  C& c; float* base; size_t words = 0;
  template <typename T> void operator()(T*& p, size_t n, const char* nm = nullptr) { p = base ? reinterpret_cast<T*>(base + words) : nullptr; words += n; c.name(p, nm); }
  size_t bytes() const { return words * sizeof(float); }
};

// The batch descriptor (camo_prepare_batch): [ row -> sample map | 1 / Nr | first 32-row tile of every sample ]
struct Desc { int* row_sample; float* inv_nr; int* tile_off; int4* tile_desc; size_t bytes; };
inline Desc desc_carve(int B, int T, void* base) {
  Desc d{};
  Carver c(base);
  d.row_sample = c.take<int>((size_t)T); d.inv_nr = c.take<float>((size_t)B); d.tile_off = c.take<int>((size_t)B + 1);
  d.tile_desc = c.take<int4>((size_t)T / 32 + B);       // one entry per block of the fused kernels' RG tile range
  d.bytes = c.bytes();
  return d;
}

// the fused row-tile kernels are written for the reference configuration
inline bool fused17_dims(const camo_dims_t& d) {
  return d.fusion_type == CAMO_FUSION_CROSS_ATTENTION && d.hidden_dim == 256 && d.num_heads == 8 && d.rg_dim == 128 && d.kg_dim == 128;
}

// ---- the fused schedule's weight shadows (bf16, MFMA-fragment order: fused_rows.h) -----------------------------------------------
// They live in the workspace, or in a caller-owned buffer (camo_shadow_bytes) that the optimizer call keeps current.  Three groups,
// each carved by one function, so both homes have one layout: carve() calls them where the groups sit in the workspace,
// shadow_carve() back to back.
struct ShadowSet {
  us16 *Wrg, *Wkg, *Wqkv_rg, *Wqkv_kg, *Wo1, *Wo2, *W1, *W2;     // forward: Wqkv_rg = [Wq1; Wk2; Wv2], what RG rows are projected with; Wqkv_kg = [Wq2; Wk1; Wv1]
  us16 *W1T, *W2T, *Wo1T, *Wo2T, *WcRgT, *WcKgT;                 // of the backward's dy . W products: dR = [dQ | dK2 | dV2] . [Wq1; Wk2; Wv2] (WcRgT), dG likewise (WcKgT)
  us16* Wf_rg; float* bf_rg;                                     // inference calls: the RG rows' folded in-projection (fused_wide2.hip, launch_fold_rg): shadow of [768 x 128], bias [768]
  size_t bytes;                                                  // (shadow_carve)
};
constexpr int kH = 256, kD = 128;     // fused17_dims
template <class C> void carve_shadows_forward(C& c, ShadowSet& s) {
  const size_t HH = (size_t)kH * kH;
  c(s.Wrg, kH * kD); c(s.Wkg, kH * kD); c(s.Wqkv_rg, 3 * HH, "Wqkv_rg"); c(s.Wqkv_kg, 3 * HH);
  c(s.Wo1, HH); c(s.Wo2, HH); c(s.W1, 2 * HH, "W1s"); c(s.W2, 2 * HH);
}
template <class C> void carve_shadows_transposed(C& c, ShadowSet& s) {
  const size_t HH = (size_t)kH * kH;
  c(s.W1T, 2 * HH, "W1T"); c(s.W2T, 2 * HH); c(s.Wo1T, HH); c(s.Wo2T, HH); c(s.WcRgT, 3 * HH, "WcRgT"); c(s.WcKgT, 3 * HH);
}
template <class C> void carve_shadows_fold(C& c, ShadowSet& s) { c(s.Wf_rg, 3 * kH * kD); c(s.bf_rg, 3 * kH); }
inline ShadowSet shadow_carve(void* base) {
  ShadowSet s{};
  Take c(base);
  carve_shadows_forward(c, s); carve_shadows_transposed(c, s); carve_shadows_fold(c, s);
  s.bytes = c.bytes();
  return s;
}

// Which parameter rows each shadow holds: rows [r0, r0 + rows) of parameter `param` ([.][cols], row-major) are rows n0.. of the plain
// shadow's N, and columns k0.. of the transposed shadow's K.  The forward builds its ShadowJobs from this table and the optimizer call
// its AdamShadowBlocks, so the shadows one leaves are the ones the other expects.  Slices of one destination are adjacent and
// ascend in n0 = k0: they are the sources of one job, in that order.
struct ShadowSlice { int param, r0, rows, cols; us16* ShadowSet::*plain; int pN, pn0; us16* ShadowSet::*trans; int tK, tk0; };
constexpr ShadowSlice k_shadow_slices[10] = {
    {CAMO_P_RG_PROJ_W, 0, kH, kD, &ShadowSet::Wrg, kH, 0, nullptr, 0, 0},
    {CAMO_P_KG_PROJ_W, 0, kH, kD, &ShadowSet::Wkg, kH, 0, nullptr, 0, 0},
    {CAMO_P_A1_IN_W, 0, kH, kH, &ShadowSet::Wqkv_rg, 3 * kH, 0, &ShadowSet::WcRgT, 3 * kH, 0},               // Wq1
    {CAMO_P_A2_IN_W, kH, 2 * kH, kH, &ShadowSet::Wqkv_rg, 3 * kH, kH, &ShadowSet::WcRgT, 3 * kH, kH},        // Wk2 | Wv2
    {CAMO_P_A2_IN_W, 0, kH, kH, &ShadowSet::Wqkv_kg, 3 * kH, 0, &ShadowSet::WcKgT, 3 * kH, 0},               // Wq2
    {CAMO_P_A1_IN_W, kH, 2 * kH, kH, &ShadowSet::Wqkv_kg, 3 * kH, kH, &ShadowSet::WcKgT, 3 * kH, kH},        // Wk1 | Wv1
    {CAMO_P_A1_OUT_W, 0, kH, kH, &ShadowSet::Wo1, kH, 0, &ShadowSet::Wo1T, kH, 0},
    {CAMO_P_A2_OUT_W, 0, kH, kH, &ShadowSet::Wo2, kH, 0, &ShadowSet::Wo2T, kH, 0},
    {CAMO_P_F1_W0, 0, 2 * kH, kH, &ShadowSet::W1, 2 * kH, 0, &ShadowSet::W1T, 2 * kH, 0},
    {CAMO_P_F2_W0, 0, 2 * kH, kH, &ShadowSet::W2, 2 * kH, 0, &ShadowSet::W2T, 2 * kH, 0}};
constexpr bool shadow_slices_ordered() {
  for (int i = 0, at = 0; i < 10; at += k_shadow_slices[i++].rows) {
    const ShadowSlice& s = k_shadow_slices[i];
    if (i && s.plain != k_shadow_slices[i - 1].plain) at = 0;
    if (s.pn0 != at || (s.trans && s.tk0 != at)) return false;
  }
  return true;
}
static_assert(shadow_slices_ordered(), "slices of one shadow must be adjacent and ascend in n0 = k0");

// ---- the workspace ---------------------------------------------------------------------------------------------------------------
// arrival-counter words of the one-launch tail behind its all-reduce buffers: 4 per group of 16 samples (misc.hip, tail_fused_kernel)
inline size_t tail_counter_words(int B) { return (size_t)4 * ((B + 15) / 16 > 0 ? (B + 15) / 16 : 1); }

struct Range { void* ptr; size_t bytes; };
struct PadRows { Range r[18]; int n; };       // the pad rows of a schedule's row-padded bf16 operands (carve: rows16)
struct HiLo {                                 // a weight of the per-sample tail as two bf16 planes in fragment order: bf16(W) and bf16(W - bf16(W))
  us16 *hi, *lo;
  us16* operator[](int low) const { return low ? lo : hi; }
};

struct Ws {
  // The zero block: everything a step accumulates into with atomics, contiguous so one clear covers it:
  //   [ Ymean H1mean Y2mean H2mean | dfused | tickets || dKV | dQ2acc | tailsum | parM ]
  // A forward that no backward follows accumulates into the part in front of `||` (zero_fwd_bytes), and into tailsum.
  float* zero_base; size_t zero_bytes, zero_fwd_bytes;
  float *Ymean, *H1mean, *Y2mean, *H2mean, *dfused, *dKV;
  int* tickets;         // [2][B] arrival counters (forward: KG->RG attention splits; backward: a sample's RG tiles)
  float* dQ2acc;        // [TK][H] fp32 sums of the KG->RG query gradient (fused backward)
  struct TailSum { float *F1sum, *hidsum, *dF1sum; unsigned int* counters; size_t bytes; } tailsum;   // the one-launch tail's all-reduce buffers [B][H | 2H | H] + its counter words
  struct ParM { float *Mrg, *Mkg, *dbrg, *dbkg; } parM;   // per stream: dQKV^T x [3H][D] and colsum(dQKV) [3H] (fused backward, parameter space)
  // forward (saved for backward)
  float *R, *G, *Q, *KV2, *KV, *Q2, *P, *P2, *O, *O2, *U, *U2, *st1, *st2, *Y, *Y2, *H1, *H2;
  float *comb, *F1, *fused, *hid, *a2;
  // backward scratch
  float *dlog, *dhid, *dF1, *dcomb, *dHm1, *dHm2, *da2;
  float *dH1, *dH2, *dY, *dY2, *dU, *dU2, *dO, *dO2, *dQ, *dQ2, *dKV2, *dS2, *dR, *dG;
  // bf16 schedule ("sched16"): a bf16 copy of every node-level GEMM operand.  Activations have their row
  // count padded to a multiple of 128 (the pad rows, `pad`, are cleared by the prep launch) so the weight-
  // gradient GEMMs contract over whole 64-row tiles without masks.  Weights: [out][in] copies for x.W^T,
  // transposed copies for dy.W, and the two in-projection slices that meet at one input concatenated
  // (WcRgT = [Wq1^T | Wk2^T | Wv2^T], WcKgT = [Wq2^T | Wk1^T | Wv1^T], both [H][3H]).
  struct H16 {
    us16 *X, *KG, *R, *G, *O, *O2, *Y, *Y2, *dH1, *dH2, *dU, *dU2, *dQKV, *dQKVkg, *dR, *dG;
    us16 *H1, *H2;   // post-ReLU/dropout FFN activations: only their sign pattern is read again (backward mask)
    us16 *Wrg, *Wkg, *Win1, *Win2, *Wo1, *Wo2, *W1, *W2, *W1T, *W2T, *Wo1T, *Wo2T, *WcRgT, *WcKgT;
    PadRows pad;
  } h;
  // fused row-tile schedule (fused_rows.h): weight shadows and the bf16 activations that cross its launches / are saved for
  // backward.  Only carved at the reference configuration (fused17_dims).
  struct F17 {
    ShadowSet sh;       // (a call that was handed external shadows: shadow_carve of those)
    us16 *X16, *KG16, *R16, *G16, *Q16, *Q2_16, *KV16, *KV2_16, *O16, *O2_16, *Y16, *Y2_16, *XH16, *XH2_16;
    float *rstd1, *rstd2, *lse2, *part; uint32_t *mask1, *mask2;
    // backward: the bf16 gradients that are weight-gradient operands, per-sample exchange buffers
    us16 *dH16, *dH2_16, *dU16, *dU2_16, *dQKV16, *dQKVkg16, *dR16, *dG16, *dO2_16;
    float *delta2, *dGpart;
    float *slabKV, *slabLN;   // the first backward half's per-block shares at small sizes (fused_rows.h, FUSED_SLAB_MAX_TILES): [RG tile][Nk][2H], [block][2H]
    PadRows pad;        // of the weight-gradient operands: their contraction runs over whole 64-row tiles
    // the per-sample tail's weights (tail_wide.h): W13, W23, Wfu0 [256 x 512], Wfu3 [256 x 256], the four heads' first layers
    // stacked [512 x 256]; and their transposes, for the tail's backward
    struct TailPlanes { HiLo W13, W23, Wfu0, Wfu3, Wh0, Wh0T, Wfu3T, Wfu0T, W13T, W23T; } tp;
  } f;
  size_t bytes;
};

enum { RG_ROWS = 0, KG_ROWS = 1 };

template <class C> Ws carve_with(C& c, const camo_dims_t& d, int B, int T, int Nk) {
  Ws w{};
  const size_t H = d.hidden_dim, TK = (size_t)B * Nk, nh = d.num_heads, Wd = 2 * d.num_classes + 2;
  if (d.fusion_type == CAMO_FUSION_CROSS_ATTENTION) {
    const size_t Fh = H / 2;
    c(w.R, T * H, "R"); c(w.G, TK * H, "G"); c(w.Q, T * H, "Q"); c(w.KV2, T * 2 * H, "KV2"); c(w.KV, TK * 2 * H, "KV"); c(w.Q2, TK * H, "Q2");
    c(w.P, T * nh * Nk, "P"); c(w.P2, T * nh * Nk, "P2"); c(w.O, T * H, "O"); c(w.O2, TK * H, "O2"); c(w.U, T * H, "U"); c(w.U2, TK * H, "U2");
    c(w.st1, T * 2); c(w.st2, TK * 2); c(w.Y, T * H, "Y"); c(w.Y2, TK * H, "Y2"); c(w.H1, T * 2 * H, "H1"); c(w.H2, TK * 2 * H, "H2");
    {
      c(w.zero_base, 0);                       // (the block's aligned start: its members follow, and c.off moves past them at the end)
      Members<C> z{c, w.zero_base};
      z(w.Ymean, B * H, "Ymean"); z(w.H1mean, B * 2 * H, "H1mean"); z(w.Y2mean, B * H, "Y2mean"); z(w.H2mean, B * 2 * H, "H2mean");
      z(w.dfused, B * H, "dfused");
      z(w.tickets, ((size_t)2 * B + 3) & ~size_t(3));
      w.zero_fwd_bytes = z.bytes();
      z(w.dKV, TK * 2 * H, "dKV"); z(w.dQ2acc, TK * H, "dQ2acc");
      Ws::TailSum& t = w.tailsum;
      const size_t t0 = z.bytes();
      z(t.F1sum, B * H); z(t.hidsum, B * 2 * H); z(t.dF1sum, B * H); z(t.counters, (tail_counter_words(B) + 3) & ~size_t(3));
      t.bytes = z.bytes() - t0;
      const size_t D = d.rg_dim;
      z(w.parM.Mrg, 3 * H * D); z(w.parM.Mkg, 3 * H * D); z(w.parM.dbrg, 3 * H); z(w.parM.dbkg, 3 * H + 8);
      w.zero_bytes = z.bytes(); c.off += w.zero_bytes;
    }
    c(w.comb, B * 2 * H, "comb"); c(w.F1, B * H, "F1"); c(w.fused, B * H, "fused"); c(w.hid, B * 4 * Fh, "hid");
    c(w.dlog, B * Wd); c(w.dhid, B * 4 * Fh, "dhid"); c(w.dF1, B * H, "dF1"); c(w.dcomb, B * 2 * H, "dcomb");
    c(w.dHm1, B * 2 * H, "dHm1"); c(w.dHm2, B * 2 * H, "dHm2");
    c(w.dH1, T * 2 * H); c(w.dH2, TK * 2 * H); c(w.dY, T * H); c(w.dY2, TK * H); c(w.dU, T * H); c(w.dU2, TK * H); c(w.dO, T * H); c(w.dO2, TK * H);
    c(w.dQ, T * H); c(w.dQ2, TK * H); c(w.dKV2, T * 2 * H); c(w.dS2, T * nh * Nk); c(w.dR, T * H); c(w.dG, TK * H);
    const size_t Tp = ((size_t)T + 127) / 128 * 128, TKp = (TK + 127) / 128 * 128, D = d.rg_dim, Dk = d.kg_dim;
    // a bf16 operand with one row per node of a stream, [rows rounded up to 128][width]; `pads`: the list whose clears cover its pad rows
    auto rows16 = [&](us16*& p, int stream, size_t width, PadRows* pads, const char* nm = nullptr) {
      const size_t rows = stream == KG_ROWS ? TK : (size_t)T, rows_p = stream == KG_ROWS ? TKp : Tp;
      c(p, rows_p * width, nm);
      if (pads) pads->r[pads->n++] = Range{p ? p + rows * width : nullptr, (rows_p - rows) * width * sizeof(us16)};
    };
    Ws::H16& h = w.h;
    rows16(h.X, RG_ROWS, D, &h.pad); rows16(h.KG, KG_ROWS, Dk, &h.pad); rows16(h.R, RG_ROWS, H, &h.pad); rows16(h.G, KG_ROWS, H, &h.pad);
    rows16(h.O, RG_ROWS, H, &h.pad); rows16(h.O2, KG_ROWS, H, &h.pad); rows16(h.Y, RG_ROWS, H, &h.pad); rows16(h.Y2, KG_ROWS, H, &h.pad);
    rows16(h.dH1, RG_ROWS, 2 * H, &h.pad); rows16(h.dH2, KG_ROWS, 2 * H, &h.pad); rows16(h.dU, RG_ROWS, H, &h.pad); rows16(h.dU2, KG_ROWS, H, &h.pad);
    rows16(h.dQKV, RG_ROWS, 3 * H, &h.pad); rows16(h.dQKVkg, KG_ROWS, 3 * H, &h.pad); rows16(h.dR, RG_ROWS, H, &h.pad); rows16(h.dG, KG_ROWS, H, &h.pad);
    c(h.Wrg, H * D); c(h.Wkg, H * Dk); c(h.Win1, 3 * H * H); c(h.Win2, 3 * H * H); c(h.Wo1, H * H); c(h.Wo2, H * H); c(h.W1, 2 * H * H); c(h.W2, 2 * H * H);
    c(h.W1T, 2 * H * H); c(h.W2T, 2 * H * H); c(h.Wo1T, H * H); c(h.Wo2T, H * H); c(h.WcRgT, 3 * H * H); c(h.WcKgT, 3 * H * H);
    rows16(h.H1, RG_ROWS, 2 * H, &h.pad); rows16(h.H2, KG_ROWS, 2 * H, &h.pad);      // (padded: they double as weight-gradient operands)
    if (fused17_dims(d)) {
      Ws::F17& f = w.f;
      carve_shadows_forward(c, f.sh);
      rows16(f.X16, RG_ROWS, D, &f.pad, "X16"); rows16(f.KG16, KG_ROWS, Dk, &f.pad); rows16(f.R16, RG_ROWS, H, &f.pad, "R16"); rows16(f.G16, KG_ROWS, H, &f.pad, "G16");
      rows16(f.Q16, RG_ROWS, H, nullptr, "Q16"); rows16(f.Q2_16, KG_ROWS, H, nullptr, "Q2_16");
      rows16(f.KV16, KG_ROWS, 2 * H, nullptr, "KV16"); rows16(f.KV2_16, RG_ROWS, 2 * H, nullptr, "KV2_16");
      rows16(f.O16, RG_ROWS, H, &f.pad, "O16"); rows16(f.O2_16, KG_ROWS, H, &f.pad, "O2_16"); rows16(f.Y16, RG_ROWS, H, &f.pad, "Y16"); rows16(f.Y2_16, KG_ROWS, H, &f.pad, "Y2_16");
      rows16(f.XH16, RG_ROWS, H, nullptr, "XH16"); rows16(f.XH2_16, KG_ROWS, H, nullptr, "XH2_16");
      c(f.rstd1, Tp, "rstd1"); c(f.rstd2, TKp, "rstd2"); c(f.lse2, (size_t)B * 8 * 16 * 2, "lse2");
      c(f.mask1, Tp * 16, "mask1"); c(f.mask2, TKp * 16, "mask2");
      c(f.part, ((size_t)T / 32 + B + 2) * 8 * FUSED_PART_FLOATS);
      carve_shadows_transposed(c, f.sh);
      rows16(f.dH16, RG_ROWS, 2 * H, &f.pad, "dH16"); rows16(f.dH2_16, KG_ROWS, 2 * H, &f.pad, "dH2_16");
      rows16(f.dU16, RG_ROWS, H, &f.pad, "dU16"); rows16(f.dU2_16, KG_ROWS, H, &f.pad, "dU2_16");
      rows16(f.dQKV16, RG_ROWS, 3 * H, &f.pad, "dQKV16"); rows16(f.dQKVkg16, KG_ROWS, 3 * H, &f.pad, "dQKVkg16");
      rows16(f.dR16, RG_ROWS, H, &f.pad, "dR16"); rows16(f.dG16, KG_ROWS, H, &f.pad, "dG16");
      rows16(f.dO2_16, KG_ROWS, H, nullptr, "dO2_16"); c(f.delta2, (size_t)B * 8 * 16, "delta2"); c(f.dGpart, TKp * H);
      auto planes = [&](HiLo& p, size_t n) { c(p.hi, n); c(p.lo, n); };
      Ws::F17::TailPlanes& t = f.tp;
      planes(t.W13, 2 * H * H); planes(t.W23, 2 * H * H); planes(t.Wfu0, 2 * H * H); planes(t.Wfu3, H * H); planes(t.Wh0, 2 * H * H);
      planes(t.Wh0T, 2 * H * H); planes(t.Wfu3T, H * H); planes(t.Wfu0T, 2 * H * H); planes(t.W13T, 2 * H * H); planes(t.W23T, 2 * H * H);
      carve_shadows_fold(c, f.sh);
      // (calls with more blocks than FUSED_SLAB_MAX_TILES take no slabs: the buffers stop growing there)
      const size_t tiles = (size_t)T / 32 + B, cap = FUSED_SLAB_MAX_TILES;
      c(f.slabKV, (tiles < cap ? tiles : cap) * Nk * 2 * H, "slabKV"); c(f.slabLN, (tiles + B < cap ? tiles + B : cap) * 2 * H, "slabLN");
    }
  } else {
    const size_t F = H / 2, Fh = F / 2, Dc = (size_t)d.rg_dim + d.kg_dim;
    c(w.zero_base, 0);
    Members<C> z{c, w.zero_base};
    z(w.comb, B * Dc, "comb");                 // [B, rg_dim+kg_dim] = the two means, zeroed then accumulated
    z(w.dfused, B * F, "dfused");
    w.zero_bytes = w.zero_fwd_bytes = z.bytes(); c.off += w.zero_bytes;
    c(w.F1, B * H, "F1"); c(w.a2, B * F); c(w.fused, B * F, "fused"); c(w.hid, B * 4 * Fh, "hid");      // (F1: a1)
    c(w.dlog, B * Wd); c(w.dhid, B * 4 * Fh, "dhid"); c(w.da2, B * F); c(w.dF1, B * H, "dF1");
  }
  w.bytes = c.bytes();
  return w;
}
inline Ws carve(const camo_dims_t& d, int B, int T, int Nk, void* base) { Take c(base); return carve_with(c, d, B, T, Nk); }

// byte offset of the buffer that carve() names `name` (camo_debug_ws_offset), -1: these dims carve none
inline int64_t ws_offset_of(const camo_dims_t& d, int B, int T, int Nk, const char* name) {
  char* const base = reinterpret_cast<char*>(4096);      // (any non-null base: nothing is dereferenced)
  Find c(base, name);
  carve_with(c, d, B, T, Nk);
  return c.hit ? static_cast<const char*>(c.hit) - base : -1;
}

}  // namespace camo_ws
