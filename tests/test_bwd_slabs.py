"""The backward's per-block slabs (csrc/fused_rows.h, Bwd1Args::slabs): at small sizes every RG tile of bwd1_kernel stores its dK | dV
share and every block its LayerNorm sums to slab rows of its own, and bwd2_kernel sums them behind the kernel boundary -- the sample's four
early blocks (four KG rows each) into dKV, four blocks at the end of its grid into the LayerNorm gradients -- where larger calls keep
the fp32 atomics.

One training step (bf16, train_raw) per case against the oracle in its bf16-operand mode after the ReLU decisions at the threshold are
settled (helpers.oracle_step_at_relu_thresholds), at the bounds the other gradient tests use: every gradient tensor that carries weight
< 1e-2, all gradients together < 2e-3, the attention blocks by helpers.assert_attention_grad_blocks_close; the tensors the slabs feed --
the k | v rows of attn1's in-projection, kg_proj, both LayerNorms' weight and bias -- are held to 1e-2 whatever their weight, and the
workspace's dKV to the oracle's dK | dV at the stage bounds of test_hip_fused.py::test_fused_backward_stage_by_stage.

Both slabs are filled with NaN bytes before the call, through the workspace offsets the library resolves: a row that no block of this
call owns and that is read anyway makes a gradient NaN.  What is left of the fill afterwards shows the launcher's choice (there is no
other read-back of it): rows of real tiles overwritten, everything else untouched -- and with the slabs in hand dKV and the
LayerNorm gradients must be the float32 sums of the owned rows in block order, bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import assert_attention_grad_blocks_close, assert_close, bf16_oracle, oracle_step_at_relu_thresholds, single_column_attentions
from oracle import fusion_oracle as FO
from oracle import params as OP

pytestmark = pytest.mark.gpu

H, NK = 256, 13
SLAB_MAX_TILES, SLAB_MAX_NR = 512, 640          # csrc/fused_rows.h: FUSED_SLAB_MAX_TILES, FUSED_SLAB_MAX_NR
SLAB_FED = {"fusion.cross_attn_rg2kg.in_proj_weight": slice(H, 3 * H), "fusion.cross_attn_rg2kg.in_proj_bias": slice(2 * H, 3 * H),
            "fusion.kg_proj.weight": slice(None), "fusion.kg_proj.bias": slice(None),
            "fusion.ln_rg.weight": slice(None), "fusion.ln_rg.bias": slice(None), "fusion.ln_kg.weight": slice(None), "fusion.ln_kg.bias": slice(None)}
# (the k rows of the in-projection's bias are zero in exact arithmetic: helpers.attention_grad_blocks)


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-30)))


def _ws_view(eng, batch, ws, name, nbytes):
    from camouflage_multimodal_amd import _lib
    off = _lib.lib().camo_debug_ws_offset(C.byref(eng.dims), batch.B, batch.T, batch.Nk, name.encode())
    assert off >= 0, name
    return ws[off:off + nbytes]


def _seq_sum_f32(rows):
    acc = np.zeros(rows.shape[1:], np.float32)
    for r in rows:
        acc = acc + r
    return acc


def run_case(nrs, dropout, pseed=6, dseed=1234):
    from test_hip_fused import close_rel, ws_f32
    from test_hip_parity import make_model, outs6, t2n
    cfg = OP.full_cfg(dict(dropout=dropout))
    m = make_model(cfg, pseed, "bf16").train()
    eng = m._engine
    B, T = len(nrs), sum(nrs)
    rgl = [OP.make_rg(n, 128, seed=300 + i) for i, n in enumerate(nrs)]
    kg = np.stack([OP.make_kg(NK, 128, seed=400 + i) for i in range(B)])
    y, e, s = OP.make_labels(B, seed=21)
    batch = eng.make_batch(torch.from_numpy(np.concatenate(rgl)).cuda(), list(nrs), torch.from_numpy(kg).cuda())
    g = eng.ensure_flat_grads(attach=True)
    g.zero_()
    ws = eng.workspace(batch, private=True)
    tiles = [(n + 31) // 32 for n in nrs]
    ntiles, tile_rows = sum(tiles), T // 32 + B
    assert ntiles <= tile_rows and tile_rows + B <= SLAB_MAX_TILES
    kv_view = _ws_view(eng, batch, ws, "slabKV", tile_rows * NK * 2 * H * 4)
    ln_view = _ws_view(eng, batch, ws, "slabLN", (tile_rows + B) * 2 * H * 4)
    kv_view.fill_(0xFF); ln_view.fill_(0xFF)                 # (uint8 views of the workspace: every float of both slabs is a NaN)
    outs, terms, _ = eng.train_raw(batch, ws, torch.from_numpy(y), torch.from_numpy(e), torch.from_numpy(s), True, dseed, eng._gtab)
    torch.cuda.synchronize()
    outs, terms = t2n(outs), t2n(terms)
    grads = {k: t2n(p.grad).copy() for k, p in m.named_parameters()}
    assert np.isfinite(outs).all() and all(np.isfinite(v).all() for v in grads.values()), "a slab row nobody wrote was read"
    slab_kv = kv_view.cpu().numpy().view(np.float32).reshape(tile_rows, NK, 2 * H)
    slab_ln = ln_view.cpu().numpy().view(np.float32).reshape(tile_rows + B, 2 * H)
    dkv = ws_f32(eng, batch, ws, "dKV", B * NK * 2 * H).reshape(B, NK, 2 * H)
    assert np.isfinite(dkv).all()

    # ---- the launcher's choice, read from what is left of the fill, and the sums the second half must have formed from the slabs
    want_kv = max(nrs) <= SLAB_MAX_NR
    written_kv = np.isfinite(slab_kv).all(axis=(1, 2)); untouched_kv = np.isnan(slab_kv).all(axis=(1, 2))
    written_ln = np.isfinite(slab_ln).all(axis=1); untouched_ln = np.isnan(slab_ln).all(axis=1)
    own_ln = np.zeros(tile_rows + B, bool); own_ln[:ntiles] = True; own_ln[tile_rows:] = True      # RG tiles, then the B KG blocks
    assert (written_ln == own_ln).all() and (untouched_ln == ~own_ln).all(), "LayerNorm slab rows: owned rows written, no other row touched"
    if want_kv:
        assert written_kv[:ntiles].all() and untouched_kv[ntiles:].all(), "dK | dV slab rows: owned rows written, no other row touched"
        t0 = 0
        for b in range(B):
            assert np.array_equal(dkv[b], _seq_sum_f32(slab_kv[t0:t0 + tiles[b]])), f"dKV of sample {b} is not the sum of its tiles' rows in tile order"
            t0 += tiles[b]
    else:
        assert untouched_kv.all(), "a sample beyond FUSED_SLAB_MAX_NR rows: dK | dV by atomics, the slab untouched"
    for name, rows, cols in (("fusion.ln_rg.weight", slice(0, ntiles), slice(0, H)), ("fusion.ln_rg.bias", slice(0, ntiles), slice(H, 2 * H)),
                             ("fusion.ln_kg.weight", slice(tile_rows, tile_rows + B), slice(0, H)), ("fusion.ln_kg.bias", slice(tile_rows, tile_rows + B), slice(H, 2 * H))):
        assert np.array_equal(grads[name], _seq_sum_f32(slab_ln[rows, cols])), f"{name} is not the sum of its slab rows in block order"

    # ---- against the oracle
    mk = lambda: bf16_oracle(OP.full_cfg(dict(dropout=dropout)), OP.make_params(cfg, pseed), nrs, False)
    ref, near, flipped = oracle_step_at_relu_thresholds(
        mk, lambda o: FO.train_step(o, FO.AdamW(o.p), rgl, kg, y, e, s, training=True, seed=dseed, debug=True), grads)
    if near:
        print("tail units at the ReLU threshold (site, sample, unit, pre-activation):", near, "taken flipped:", flipped)
    want = ref["raw_grads"]
    den = sum(float((want[k].astype(np.float64) ** 2).sum()) for k in grads)
    total = float(np.sqrt(sum(float(((grads[k].astype(np.float64) - want[k]) ** 2).sum()) for k in grads) / den))
    per = sorted(((_rel(grads[k], want[k]), k) for k in grads if (want[k].astype(np.float64) ** 2).sum() > 1e-6 * den), reverse=True)
    fed = sorted(((_rel(grads[k][sl], want[k][sl]), k) for k, sl in SLAB_FED.items()), reverse=True)
    cat = lambda k: np.concatenate([d[k] for d in ref["dbg"]])
    want_dkv = np.concatenate([cat("dKk"), cat("dVk")], axis=1)
    print(f"nrs={nrs} dropout={dropout}: global relative gradient error {total:.5f}; worst tensor {per[0][1]} {per[0][0]:.4f}; slab-fed tensors: "
          + ", ".join(f"{k.replace('fusion.', '')} {r:.4f}" for r, k in fed) + f"; dKV max |err| / max |want| "
          f"{np.abs(dkv.reshape(B * NK, 2 * H) - want_dkv).max() / max(np.abs(want_dkv).max(), 1e-30):.4f}")
    assert_close(outs, outs6(ref["outs"]), 5e-4, 0, "outputs vs the bf16-operand oracle")
    assert_close(terms, ref["loss_terms"], 2e-3, 1e-3, "loss terms")
    assert total < 2e-3, (total, per[:4])
    assert per[0][0] < 1e-2, per[:4]
    assert fed[0][0] < 1e-2, fed
    close_rel(dkv.reshape(B * NK, 2 * H), want_dkv, 2e-2, "dK | dV sums", 3e-3, flips=2e-3)
    assert_attention_grad_blocks_close(grads, want, what=f"nrs={nrs} dropout={dropout}", single_column=single_column_attentions(nrs, NK))


@pytest.mark.parametrize("dropout", [0.0, 0.3])
@pytest.mark.parametrize("nrs", [[5], [32, 33, 64], [530, 303]], ids=["one-partial-tile", "exact-one-row-two-full", "17-and-10-tiles"])
def test_slab_paths_match_the_oracle(nrs, dropout):
    """One partial tile; an exact tile, a second tile of one row, two full tiles; 17 and 10 tiles, the ends of the Nr histogram (two
    passes and one pass of the KG block's sum)."""
    run_case(nrs, dropout)


@pytest.mark.parametrize("max_nr", [SLAB_MAX_NR, SLAB_MAX_NR + 1], ids=["640-slabs", "641-atomics"])
def test_both_sides_of_the_switch(max_nr):
    """The largest sample that sends dK | dV through the slabs (20 tiles: two full passes of the KG block's sum) and the first that keeps
    the atomics (21 tiles); the LayerNorm sums take their slab on both sides.  run_case reads the choice from the sentinel fill."""
    run_case([max_nr, 33], 0.3)
