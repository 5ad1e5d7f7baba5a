"""The two in-kernel sites of the loss, reached by size: loss_sample<FAST> inside the one-launch tail (tail_fused_kernel, the
benchmarked path) and the library-math loss_sample inside heads_loss_kernel<ACC> -- each against oracle/f64_refs.loss_f64
EVALUATED ON THE ``outs`` THE CALL RETURNED, so nothing upstream (bf16 rounding, ReLU decisions, summation order) enters the
comparison.  Needs an MI355X.

A model with seed-style parameters in which only the four ``{head}.3.bias`` tensors change: a bias shifts that head's logits for
every sample and amplifies nothing upstream.  Shift patterns: none; mask / instance +-6 and +-15 (class 0 up, every other class
down: a sample labelled 0 is saturated right, any other saturated wrong); edge +-12; score pre-sigmoid +-10 and +-30.

Per case: camo_debug_plan must report the intended loss site first; then one native training call (train_raw: it returns the
outs; gradients raw, nothing clipped) and, against loss_f64 on those outs: the loss terms under the per-element bound, pred
exactly, and the gradients of the four .3.bias tensors, which are exactly sum_b d_pre[b] over that head's columns -- bound: the
sum of the elements' bounds + B u sum_b |d_pre| for the float32 summation (any order).

Planned sites (camo_debug_plan, asserted): bf16 at default dims with B in {1, 5, 16} x C in {2, 8} and B = 17 (two 16-sample
groups: the one-launch tail takes up to 48 samples) -> CAMO_LOSS_TAIL, FAST; f32 at B in {17, 70, 300} and bf16 at B in {70, 300}
(default dims, C = 2: ACC, S = 1 / 2 / 4) and f32 on small dims at C in {9, 64} x B in {17, 70, 300} (ACC off) -> CAMO_LOSS_HEADS.

The score column: sigmoid_f64(pre) with pre = logit(baseline outs) + the shift, where the baseline outs are well conditioned
(1e-3 < outs < 1 - 1e-3); bound s (1 - s) (d exp + d pre) + 3 u s with d exp = (2 + |pre| log2 e) ulp for __expf and
d pre = the recovery's own error + u |pre0| + u |pre| + 256 u: two calls differ in the pre-activation by the summation order of
the fp32 atomics upstream and of the 128-term dot product (n u sum |terms|, sum |terms| <~ 1).  Everywhere: outs in [0, 1],
monotone in the shift, finite gradients.

Largest observed error / bound (MI355X):  
  one-launch tail, FAST                terms 0.28, bias gradients 0.15
  heads_loss_kernel<ACC on>            terms 0.34, bias gradients 0.08
  heads_loss_kernel<ACC off>           terms 0.31, bias gradients 0.10
  score sigmoid (__expf), both sites   0.13
"""
import ctypes as C_

import numpy as np
import pytest
import torch

from oracle import f64_refs as R
from oracle import params as OP
from test_hip_parity import make_model
from test_size_switches import SMALL_A, _f32_case

pytestmark = pytest.mark.gpu

LOSS_TAIL, LOSS_HEADS = 1, 2                      # CAMO_LOSS_TAIL / CAMO_LOSS_HEADS (include/camo_fusion.h)
HEADS = ("mask_head", "instance_head", "edge_head", "score_head")
NK = 13
SEED = 0x1234ABCD5678EF01

# id -> (dims overrides, precision, B, C, intended loss site)
CONFIGS = {}
for _B in (1, 5, 16):
    for _C in (2, 8):
        CONFIGS[f"tail-bf16-B{_B}-C{_C}"] = ({}, "bf16", _B, _C, LOSS_TAIL)
CONFIGS["tail-bf16-B17-C2"] = ({}, "bf16", 17, 2, LOSS_TAIL)
for _B in (17, 70, 300):
    CONFIGS[f"heads-f32-B{_B}-C2"] = ({}, "f32", _B, 2, LOSS_HEADS)
    if _B != 17:
        CONFIGS[f"heads-bf16-B{_B}-C2"] = ({}, "bf16", _B, 2, LOSS_HEADS)
    for _C in (9, 64):
        CONFIGS[f"heads-f32-small-B{_B}-C{_C}"] = (SMALL_A, "f32", _B, _C, LOSS_HEADS)

# pattern -> (head, shift of class 0 / of the single output, shift of every other class)
PATTERNS = {"baseline": None, "mask+-6": ("mask_head", 6.0, -6.0), "mask+-15": ("mask_head", 15.0, -15.0),
            "instance+-6": ("instance_head", 6.0, -6.0), "instance+-15": ("instance_head", 15.0, -15.0),
            "edge+12": ("edge_head", 12.0, 0.0), "edge-12": ("edge_head", -12.0, 0.0),
            "score+10": ("score_head", 10.0, 0.0), "score-10": ("score_head", -10.0, 0.0),
            "score+30": ("score_head", 30.0, 0.0), "score-30": ("score_head", -30.0, 0.0)}

_STATE = {}                   # config id -> dict(model, inputs, base biases, results per pattern)
WORST = {}


def _setup(cid):
    if cid in _STATE:
        return _STATE[cid]
    over, prec, B, C, _ = CONFIGS[cid]
    cfg = OP.full_cfg(dict(over, num_classes=C))
    model = make_model(cfg, 6, prec).train()
    nrs = [8 + (3 * b) % 25 for b in range(B)]
    rg = torch.from_numpy(np.concatenate([OP.make_rg(n, cfg["rg_dim"], seed=300 + b) for b, n in enumerate(nrs)])).cuda()
    kg = torch.from_numpy(np.stack([OP.make_kg(NK, cfg["kg_dim"], seed=400 + b) for b in range(B)])).cuda()
    _, _, s = OP.make_labels(B, seed=50 + B)
    b = np.arange(B)
    e = (b % 3 == 0).astype(np.float32)                                             # (both edge labels from B = 2 on)
    y = np.where(b % 2 == 0, 0, 1 + (b // 2) % max(C - 1, 1)).astype(np.int64)      # half the samples class 0, the rest walk the others
    params = dict(model.named_parameters())
    base = {h: params[f"{h}.3.bias"].detach().cpu().numpy().copy() for h in HEADS}
    _STATE[cid] = st = dict(model=model, cfg=cfg, nrs=nrs, rg=rg, kg=kg, y=y, e=e, s=s, params=params, base=base, res={})
    return st


def _run(cid, pattern):
    """One training call of config ``cid`` with the shift ``pattern`` -> dict(outs, terms, pred, bias grads, shift); memoised."""
    from camouflage_multimodal_amd import _lib
    st = _setup(cid)
    if pattern in st["res"]:
        return st["res"][pattern]
    _, prec, B, C, site = CONFIGS[cid]
    eng = st["model"]._engine
    shift = {h: np.zeros_like(v, np.float64) for h, v in st["base"].items()}
    with torch.no_grad():
        for h in HEADS:
            new = st["base"][h].copy()
            if PATTERNS[pattern] is not None and PATTERNS[pattern][0] == h:
                _, a0, a1 = PATTERNS[pattern]
                new = (new.astype(np.float64) + np.where(np.arange(len(new)) == 0, a0, a1)).astype(np.float32)
            shift[h] = new.astype(np.float64) - st["base"][h].astype(np.float64)            # (the shift in effect, exactly)
            st["params"][f"{h}.3.bias"].copy_(torch.from_numpy(new).cuda())
    # the plan first: a case that silently takes another path is a failure, not a pass
    plan = _lib.CamoPlan()
    _lib.check(_lib.lib().camo_debug_plan(C_.byref(eng.dims), 3, B, sum(st["nrs"]), NK, max(st["nrs"]),
                                          _lib.PREC_BF16 if prec == "bf16" else _lib.PREC_F32, 0, _lib.CALL_TRAIN, -1, C_.byref(plan)),
               "camo_debug_plan")
    assert plan.loss == site, f"{cid}: planned loss site {plan.loss}, intended {site}"
    batch = eng.make_batch(st["rg"], st["nrs"], st["kg"])
    g = eng.ensure_flat_grads(attach=True)
    g.zero_()
    outs, terms, pred = eng.train_raw(batch, eng.workspace(batch), torch.from_numpy(st["y"]), torch.from_numpy(st["e"]),
                                      torch.from_numpy(st["s"]), True, SEED, eng._gtab)
    torch.cuda.synchronize()
    n = lambda t: t.detach().cpu().numpy().copy()
    res = dict(outs=n(outs), terms=n(terms), pred=n(pred), shift=shift,
               bias_grad={h: n(st["params"][f"{h}.3.bias"].grad) for h in HEADS},
               finite=bool(torch.isfinite(g).all()))
    st["res"][pattern] = res
    return res


def _assert_under(got, want, bound, what, tag):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), f"{what}: non-finite"
    ratio = np.abs(got - want) / bound
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio[i] <= 1.0, f"{what}{i}: got {got[i]!r} want {want[i]!r}: |err| {abs(got[i] - want[i]):.3e} = {ratio[i]:.2f} x bound {bound[i]:.3e}"
    WORST[tag] = max(WORST.get(tag, 0.0), float(ratio[i]))


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("cid", list(CONFIGS))
def test_in_kernel_loss_matches_float64_reference_on_its_own_outs(cid, pattern):
    _, prec, B, C, site = CONFIGS[cid]
    st = _setup(cid)
    r = _run(cid, pattern)
    assert r["finite"], "non-finite gradient"
    fast = site == LOSS_TAIL
    ref = R.loss_f64(r["outs"], st["y"], st["e"], st["s"], C, fast=fast)
    tag = ("tail FAST" if fast else f"heads_loss_kernel<ACC={'on' if C <= 8 else 'off'}>")
    _assert_under(r["terms"], ref["terms"], ref["terms_bound"], f"{cid} {pattern} terms", tag + " terms")
    assert np.array_equal(r["pred"], ref["pred"])
    cols = dict(mask_head=slice(0, C), instance_head=slice(C, 2 * C), edge_head=slice(2 * C, 2 * C + 1), score_head=slice(2 * C + 1, 2 * C + 2))
    for h in HEADS:
        d = ref["d_pre"][:, cols[h]]
        bound = ref["d_pre_bound"][:, cols[h]].sum(0) + (B * R.U * np.abs(d).sum(0) if B > 1 else 0.0)
        _assert_under(r["bias_grad"][h], d.sum(0), bound, f"{cid} {pattern} grad {h}.3.bias", tag + " bias gradients")
    # the regime the pattern is meant to reach, on the reference
    if PATTERNS[pattern] is not None and B >= 5:
        head = PATTERNS[pattern][0]
        o = r["outs"].astype(np.float64)
        if head in ("mask_head", "instance_head"):
            lg = o[:, cols[head]]
            p = np.exp(lg - lg.max(1, keepdims=True)); p /= p.sum(1, keepdims=True)
            pt = p[np.arange(B), st["y"]]
            assert pt.max() > 0.99 and pt.min() < 0.01, (pt.min(), pt.max())             # saturated right AND saturated wrong
        elif head == "edge_head":
            right = (o[:, 2 * C] > 0) == (st["e"] > 0.5)
            assert np.abs(o[:, 2 * C]).min() > 8 and right.any() and (~right).any()
        else:
            sc = o[:, 2 * C + 1]
            assert (sc < 1e-3).all() or (sc > 1 - 1e-3).all()
    print(f"{cid} {pattern}: planned onto loss site {site}; largest error / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_score_column_is_the_sigmoid_of_the_shifted_pre_activation(cid):
    _, prec, B, C, site = CONFIGS[cid]
    base = _run(cid, "baseline")
    s0 = base["outs"][:, -1].astype(np.float64)
    assert ((s0 >= 0) & (s0 <= 1)).all()
    ok = (s0 > 1e-3) & (s0 < 1 - 1e-3)
    assert ok.any()
    pre0 = np.log(s0[ok]) - np.log1p(-s0[ok])
    dexp = lambda x: (2.0 + np.abs(x) * R.LOG2E) * R.ULP
    dpre0 = dexp(pre0) + 3.0 * R.U / (1.0 - s0[ok]) + 3.0 * R.U / s0[ok]               # d s0 = s0 (1 - s0) d exp + 3 u s0, / the slope; + logit of a rounded s0
    prev = None
    for pattern in ("score-30", "score-10", "baseline", "score+10", "score+30"):
        r = _run(cid, pattern)
        sc = r["outs"][:, -1].astype(np.float64)
        assert r["finite"] and np.isfinite(r["terms"]).all()
        assert ((sc >= 0) & (sc <= 1)).all(), pattern
        if prev is not None:
            assert (sc >= prev).all(), f"{pattern}: the score is not monotone in the shift"
        prev = sc
        if pattern == "baseline":
            continue
        pre = pre0 + r["shift"]["score_head"][0]
        want = R.sigmoid_f64(pre)
        bound = 2.0 * (want * (1.0 - want) * (dexp(pre) + dpre0 + R.U * np.abs(pre0) + R.U * np.abs(pre) + 256.0 * R.U) + 3.0 * R.U * want) \
            + R.ULP * want + R.TINY
        _assert_under(sc[ok], want, bound, f"{cid} {pattern} score", "score sigmoid (__expf)")
    print(f"{cid}: score sigmoid largest error / bound {WORST.get('score sigmoid (__expf)', 0.0):.3f}")


@pytest.mark.parametrize("C", [9, 64])
def test_f32_training_step_many_classes_small_dims(C):
    """A whole f32 training step against the oracle at C = 9 and C = 64 (small dims, dropout 0.3; heads_loss_kernel<ACC off>) at
    the bounds of the other f32 dropout cases, with labels that walk the classes: the alpha rule for classes >= 2 end to end."""
    nrs = [40, 1, 130]
    y = np.array([C - 1, 1, 2], np.int64)
    _f32_case(OP.full_cfg(dict(SMALL_A, num_classes=C, dropout=0.3)), 3, nrs, 17, y=y)
