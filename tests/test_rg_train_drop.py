"""Loss and gradients of the region-graph GNN WITH DROPOUT (include/camo_rg_train_drop.h) against
tests/rg_train_drop_ref.py, in both batch-norm modes (0: frozen statistics, 1: batch statistics).

PARITY UNPINNED (the reference tree, torch_geometric and an RG checkpoint are absent): the header is the definition, the torch
restatement the checker.  CPU tests tie the restatement at rate 0 to tests/rg_train_ref.py and tests/rg_train_bn_ref.py, its masks to
oracle.fusion_oracle.dropout_keep and the threshold rule of csrc/common.h's make_drop, and the library's argument checks to the header.
GPU tests hold the four loss figures and the 32 gradients (batch statistics: batch_stats and the eight updated running statistics too)
to float64 with the project's rule,

    e = max|g - g64| / max(max|g64|, 1e-12)  <=  8 e32 + 2e-6,

e32 being the same error of torch-CPU float32 autograd of the same restatement ON THE SAME MASKS, computed in the same test; under batch
statistics the four conv-bias gradients are compared as bytes against +0.0.  Every case first asserts ON THE CPU REFERENCE that none of
the nine pre-activation taps lies within 1e-4 max|tensor| of 0.  A mask changes every pre-activation above it, so the margin is a
property of (inputs, mode, rates, dropout seed): the parameter seeds and the dropout seeds below were found by a search on the CPU for
that condition and are fixed.

Cases: "real" (23 nodes, hidden 128, heads 4: each class alone at 0.3 and all three at (0.2, 0.3, 0.5)), "tail" (70 rows: the row
blocks of 64 and 6), "wide" (9 nodes, hidden 192: the CPL = 8 DROP instantiations), "many" (1082 nodes = 16 copies of three graphs and a
remainder, as tests/test_rg_train_bn.py builds them: element indices past one block of every kernel, two nodes to a thread in the loss
kernel).  In "many" the copies share weights but NOT masks, so nothing is gained from a copy's margin: the margin is asserted on the
whole batch, where every pre-activation above the first dropout site -- about 5.5 hidden per node -- has to clear 1e-4 on its own.  A
CPU search at N = 1082 found no clear draw in 400 000 dropout seeds at hidden 4 under frozen statistics with the first parameter seed,
one in a thousand with another, and none in 30 000 over 30 parameter seeds under batch statistics (whose standardised pre-activations
always have mass at 0); at hidden 2 a clear draw is one in 16 under batch statistics, so "many" runs at hidden 2, heads 2 (3 head units)
in both modes.  What "many" is for -- 17 row blocks, element indices and node counts past one block of every kernel -- does not depend
on hidden; hidden 128 and 192 are covered by "real" and "wide".
(In "many" under frozen statistics the float64 gradient of conv1.att_dst is zero to rounding -- max|g64| = 2.3e-19 beside 2.5e-4 for
conv1.att_src -- so its e and e32 are ratios of rounding noise, 43 against 91 on one MI355X run: the rule holds it and says nothing.  Largest e / e32 over the other quantities of that configuration: 8.9e-7 / 2.4e-6.)
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import rg_detect_ref as R
import rg_train_bn_ref as BR
import rg_train_drop_ref as DR
import rg_train_ref as TR
from conftest import ROOT
from oracle import rg_gnn_oracle as RO
from oracle.fusion_oracle import dropout_keep
from rg_train_calls import direct, refuse
from test_rg_train import NAMES, _bits, _csr_pair, _data, _err, _model, _targets
from test_rg_train_bn import BIAS_NAMES, LOSS_KEYS, STAT_NAMES, _graph, _running, _sizes

ALL = (0.2, 0.3, 0.5)
# name: (graph kind, n, hidden, heads, classes)
SHAPES = {
    "real": ("grid", 23, 128, 4, 2),
    "tail": ("grid", 70, 32, 1, 2),
    "wide": ("grid", 9, 192, 2, 2),
    "many": ("many", 1082, 2, 2, 2),
    "small": ("grid", 23, 32, 2, 2),            # tests/test_rg_finetune_drop.py's: three consecutive dropout seeds have to be clear
}
# (case, mode): seed of the graph, the parameters and the targets -- the attention scores and the first batch norm's output do not
# depend on dropout, so this seed alone has to clear them in its mode
PARAM_SEEDS = {
    ("real", 0): 343, ("real", 1): 45,
    ("tail", 0): 0, ("tail", 1): 720,
    ("wide", 0): 1, ("wide", 1): 224,
    ("many", 0): 0, ("many", 1): 0,
    ("small", 1): 17,
}
# (case, mode, (p_conv, p_shared, p_head)): dropout seed; flip margins on the float64 reference in the comments
CONFIGS = {
    ("real", 0, (0.3, 0.0, 0.0)): 231,       # 1.09e-4
    ("real", 0, (0.0, 0.3, 0.0)): 0,         # 1.41e-4
    ("real", 0, (0.0, 0.0, 0.3)): 0,         # 1.41e-4 (the heads' dropout is above every tap: the margin of the inputs)
    ("real", 0, ALL): 19,                    # 1.47e-4
    ("tail", 0, ALL): 42,                    # 1.13e-4
    ("wide", 0, ALL): 15,                    # 1.32e-4
    ("many", 0, ALL): 0,                     # 2.03e-4
    ("real", 1, (0.3, 0.0, 0.0)): 667,       # 1.08e-4
    ("real", 1, (0.0, 0.3, 0.0)): 18,        # 1.93e-4
    ("real", 1, (0.0, 0.0, 0.3)): 0,         # 1.10e-4 (the margin of the inputs)
    ("real", 1, ALL): 287,                   # 1.57e-4
    ("tail", 1, ALL): 31,                    # 1.27e-4
    ("wide", 1, ALL): 90,                    # 1.51e-4
    ("many", 1, ALL): 18,                    # 1.15e-4
}


def _key_id(key):
    case, mode, rates = key
    return f"{case}-{'batch' if mode else 'frozen'}-{'-'.join(f'{v:g}' for v in rates)}"


@functools.lru_cache(maxsize=None)
def _inputs(case, mode, param_seed=None):
    """Graph, parameters and targets of a case in a mode, drawn as tests/test_rg_train_bn.py draws them; never written to."""
    kind, n, hidden, heads, nc = SHAPES[case]
    seed = PARAM_SEEDS[(case, mode)] if param_seed is None else param_seed
    p = dict(RO.make_params(seed, 15, hidden, heads))
    p.update(R.make_head_params(seed + 1, hidden, nc))
    x, ei, ew = _graph(kind, n, seed)
    rs = np.random.RandomState(seed + 1000)
    mt = rs.randint(0, nc, size=n).astype(np.int32)
    it = rs.randint(0, nc, size=n).astype(np.int32)
    et = rs.uniform(0, 1, size=n).astype(np.float32)
    if kind == "many":                # per node over the whole batch, so the copies of a graph do not have equal gradients
        mt[rs.uniform(size=n) < 0.1] = -1
        et[rs.uniform(size=n) < 0.1] = -1.0
        mt[1030], et[1040] = -1, -1.0
    for a in list(p.values()) + [x, ei, ew, mt, it, et]:
        a.setflags(write=False)
    return dict(p=p, x=x, ei=ei, ew=ew, mt=mt, it=it, et=et, hidden=hidden, heads=heads, nc=nc, n=n, sizes=_sizes(kind))


def _ref(c, rates, seed, mode, dtype=torch.float64, **kw):
    return DR.loss_and_grads(c["p"], c["x"], c["ei"], c["ew"], c["mt"], c["it"], c["et"], c["heads"], c["nc"], rates, seed, bool(mode),
                             dtype=dtype, **kw)


@functools.lru_cache(maxsize=None)
def _case(key):
    """Inputs and both CPU references (float64, float32 on the same masks) of a configuration, computed once; never written to."""
    case, mode, rates = key
    c = dict(_inputs(case, mode))
    seed = CONFIGS[key]
    masks = {}
    l64, g64, margin, bs64, run64 = _ref(c, rates, seed, mode, masks=masks)
    l32, g32, _, bs32, run32 = _ref(c, rates, seed, mode, dtype=torch.float32)
    c.update(l64=l64, g64=g64, margin=margin, bs64=bs64, run64=run64, l32=l32, g32=g32, bs32=bs32, run32=run32, masks=masks, seed=seed,
             rates=rates, mode=mode)
    return c


def _bound(e32):
    return 8 * e32 + 2e-6


# ---- CPU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["real", "tail"])
def test_at_rate_zero_the_restatement_is_both_older_restatements(case):
    """Losses and all 32 gradients to 1e-12 relative; batch statistics and running updates too."""
    for mode in (0, 1):
        c = _inputs(case, mode)
        args = (c["p"], c["x"], c["ei"], c["ew"], c["mt"], c["it"], c["et"], c["heads"], c["nc"])
        l, g, margin, bs, run = _ref(c, (0.0, 0.0, 0.0), 12345, mode)
        if mode:
            wl, wg, wm, wbs, wrun = BR.loss_and_grads(*args)
            assert np.abs(bs - wbs).max() <= 1e-12 * np.abs(wbs).max()
            assert all(np.abs(run[k] - wrun[k]).max() <= 1e-12 * np.abs(wrun[k]).max() for k in STAT_NAMES)
        else:
            wl, wg, wm = TR.loss_and_grads(*args)
            assert bs is None and run is None
        assert abs(margin - wm) <= 1e-12 * wm
        assert all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(l, wl))
        top = max(float(np.abs(v).max()) for v in wg.values())
        for k in NAMES:
            assert np.abs(g[k] - wg[k]).max() <= 1e-12 * max(float(np.abs(wg[k]).max()), 1e-3 * top), (mode, k)


def test_masks_are_dropout_keep_on_the_headers_indices_and_keep_counts_are_binomial():
    c = _inputs("real", 0)
    n, hidden, seed, p = c["n"], c["hidden"], 77, 0.3
    units = 3 * (hidden // 2)
    assert n * hidden >= 2944
    masks = {}
    _ref(c, (p, p, p), seed, 0, want_grads=False, masks=masks)
    assert sorted(masks) == [32, 33, 34, 35, 36, 37]
    for site, keep in masks.items():
        cols = units if site == 37 else hidden
        assert keep.shape == (n, cols)
        for r, col in ((0, 0), (3, 5), (n - 1, cols - 1)):                     # element (n, c) is index n * cols + c of its site
            assert bool(keep[r, col]) == bool(dropout_keep(seed, site, np.array([r * cols + col], np.uint64), np.float32(p))[0])
        assert np.array_equal(keep.reshape(-1), dropout_keep(seed, site, np.arange(n * cols, dtype=np.uint64), np.float32(p)))
        cnt, tot = int(keep.sum()), n * cols
        assert abs(cnt - (1 - p) * tot) <= 5 * np.sqrt(tot * p * (1 - p)), (site, cnt, tot)
    assert len({m.tobytes() for s, m in masks.items() if s != 37}) == 5         # the sites draw different masks
    assert DR.multiplier(0.3) == float(np.float32(1) / (np.float32(1) - np.float32(0.3))) and DR.multiplier(0.5) == 2.0


def _fmix32(x):
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13); x = (x * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    return x ^ (x >> np.uint64(16))


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5, 1 - 2.0 ** -24])
def test_the_threshold_rule_is_dropout_keep(p):
    """make_drop's rule (csrc/common.h, the header's text): keep iff hash >= ceil(p 2^24) << 8, p the fp32 rate, on 10^6 indices."""
    seed, site = 0x123456789ABCDEF, 33
    idx = np.arange(10 ** 6, dtype=np.uint64) * np.uint64(4099) % np.uint64(1 << 32)
    p32 = float(np.float32(p))
    t24 = int(np.ceil(p32 * 16777216.0))                                           # exact: p32 2^24 is a double without rounding
    thr = 0xFFFFFFFF if t24 >= 1 << 24 else t24 << 8
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    h = _fmix32(((idx + np.uint64((site * 0x85EBCA77 + lo) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)) ^ np.uint64(hi))
    want = dropout_keep(seed, site, idx, np.float32(p))
    assert np.array_equal(h >= np.uint64(thr), want)
    assert abs(int(want.sum()) - (1 - p32) * idx.size) <= 5 * np.sqrt(idx.size * p32 * (1 - p32)) + 1


def test_header_symbols_sites_binding_and_abi_version():
    from camouflage_multimodal_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "camo_rg_train_drop.h")).read()
    assert "PARITY UNPINNED" in hdr and "train.py" in hdr and "0x85EBCA77" in hdr
    sites = {k: int(v) for k, v in re.findall(r"#define (CAMO_RGT_SITE_\w+) (\d+)", hdr)}
    assert sites == {"CAMO_RGT_SITE_CONV0": DR.SITE_CONV0, "CAMO_RGT_SITE_SHARED": DR.SITE_SHARED, "CAMO_RGT_SITE_HEADS": DR.SITE_HEADS}
    common = open(os.path.join(ROOT, "camouflage_multimodal_amd", "csrc", "common.h")).read()
    assert re.search(r"SITE_RGT_CONV0 = 32\b", common) and re.search(r"SITE_RGT_SHARED = 36\b", common) and re.search(r"SITE_RGT_HEADS = 37\b", common)
    assert _lib.symbols("camo_rg_train_drop.h") == ("camo_rg_train_drop_workspace_bytes", "camo_rg_loss_backward_drop")
    assert _lib.ABI_VERSION == 13 and _lib.lib().camo_abi_version() == 13
    assert "struct" not in re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)


def test_argument_checks_match_the_header():
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()

    def call(mode=1, rates=(0.1, 0.2, 0.3), ws_bytes=8, **kw):       # fake pointers: every check runs on the host before any launch
        return refuse("camo_rg_loss_backward_drop", mode=mode, rates=rates, ws_bytes=ws_bytes, seed=7, **kw)[0]

    E_ARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3
    for mode in (0, 1):
        assert call(mode) == E_WORKSPACE                                         # everything but the workspace is in order
        for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
            for slot in range(3):
                rates = [0.1, 0.2, 0.3]
                rates[slot] = bad
                assert call(mode, tuple(rates)) == E_ARG, (mode, bad, slot)
                assert b"dropout rates" in L.camo_last_error()
        assert call(mode, (0.0, 0.0, 0.0)) == E_WORKSPACE and call(mode, (float(np.float32(1 - 2.0 ** -24)),) * 3) == E_WORKSPACE
    assert call(0, running=True) == E_ARG and b"must be null" in L.camo_last_error()
    assert call(0, stats=True) == E_ARG and b"must be null" in L.camo_last_error()
    assert call(1, running=True, stats=True) == E_WORKSPACE
    assert call(1, running=True, momentum=0.0) == E_ARG and b"momentum" in L.camo_last_error()   # the mode's own checks follow
    assert call(2) == E_ARG and call(-1) == E_ARG and b"batch_stats_mode" in L.camo_last_error()
    assert call(1, N=1, E=1) == E_UNSUPPORTED and call(0, N=1, E=1) == E_WORKSPACE                   # N >= 2 is batch statistics' own
    assert call(0, hidden=127) == E_UNSUPPORTED and call(0, heads=9) == E_UNSUPPORTED
    # N (3 hidden / 2) < 2^32: hidden 512 -> 768 units; 2^32 / 768 = 5592405.33
    assert call(0, hidden=512, N=5592406, E=5592406) == E_UNSUPPORTED and b"2^32" in L.camo_last_error()
    assert call(0, hidden=512, N=5592405, E=5592405) == E_WORKSPACE
    d = _lib.CamoRgDims(15, 128, 4)
    for n, e in ((23, 100), (70, 400), (1, 1)):
        assert L.camo_rg_train_drop_workspace_bytes(ctypes.byref(d), 2, n, e, 0) == L.camo_rg_train_workspace_bytes(ctypes.byref(d), 2, n, e)
        assert L.camo_rg_train_drop_workspace_bytes(ctypes.byref(d), 2, n, e, 1) == L.camo_rg_train_bn_workspace_bytes(ctypes.byref(d), 2, n, e)
    assert L.camo_rg_train_drop_workspace_bytes(None, 2, 23, 100, 0) == 0 and L.camo_rg_train_drop_workspace_bytes(ctypes.byref(d), 2, 23, 100, 0) > 0


def test_bad_rates_and_cpu_tensors_raise_before_any_device_work():
    from camouflage_multimodal_amd import RegionGraphData, RegionGraphFineTuner, RegionGraphGNN
    from camouflage_multimodal_amd._lib import CamoError
    c = _inputs("tail", 1)
    m = RegionGraphGNN(hidden_channels=32, num_classes=2, heads=1)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    data = RegionGraphData(torch.from_numpy(c["x"].copy()), torch.from_numpy(c["ei"].copy()), torch.from_numpy(c["ew"].copy())[:, None])
    t = (torch.from_numpy(c["mt"].copy()), torch.from_numpy(c["it"].copy()), torch.from_numpy(c["et"].copy()))
    for bad in (-0.1, 1.0, float("nan"), (0.1, 0.2), (0.1, 0.2, 1.0), "much"):
        for bs in (False, True):
            with pytest.raises((CamoError, ValueError), match="dropout"):
                m.loss_and_gradients(data, *t, batch_stats=bs, dropout=bad)
        with pytest.raises((CamoError, ValueError), match="dropout"):
            RegionGraphFineTuner(m, dropout=bad)
    with pytest.raises(ValueError, match="seed"):
        m.loss_and_gradients_csr(data.x, (None,) * 3, (None,) * 3, *t, dropout=0.1, seed=-1)
    for bs in (False, True):
        with pytest.raises(CamoError):                                         # CPU tensors
            m.loss_and_gradients(data, *t, batch_stats=bs, dropout=0.3, seed=5)
    assert all(p.grad is None for p in m.parameters())
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert m._dropout_rates(None) is None and m._dropout_rates(0) is None and m._dropout_rates((0, 0.0, 0)) is None
    assert m._dropout_rates(0.5) == (0.5, 0.5, 0.5) and m._dropout_rates([0, 0.25, 0]) == (0.0, 0.25, 0.0)
    tuner = RegionGraphFineTuner(m, dropout=(0.1, 0.2, 0.3), seed=11)
    assert tuner.dropout == (0.1, 0.2, 0.3) and tuner.seed == 11 and tuner.step_count == 0
    assert RegionGraphFineTuner(m).dropout is None and RegionGraphFineTuner(m).seed == 0
    with pytest.raises(CamoError, match="training mode logits"):
        m.train()(data)                                                        # forward in training mode keeps raising


def test_the_wrapper_picks_its_entry_by_batch_stats_rates_and_pixel():
    """At neutral extras the four entries give the same bytes, so no GPU test sees a wrong choice: the rule is held here, on all eight
    combinations, and composed with _dropout_rates, whose zeros must not reach the dropout entry."""
    from camouflage_multimodal_amd import RegionGraphGNN
    entry, rates_of = RegionGraphGNN._training_entry, RegionGraphGNN._dropout_rates
    pixel = (None, [0, 23], 15, 1.0)                                          # (given or not: its fields are not looked at)
    for bs in (False, True):
        assert entry(bs, None, None) == ("camo_rg_loss_backward_bn" if bs else "camo_rg_loss_backward")
        assert entry(bs, ALL, None) == "camo_rg_loss_backward_drop"
        assert entry(bs, None, pixel) == entry(bs, ALL, pixel) == "camo_rg_loss_backward_pixel"
        for zero in (None, 0, 0.0, (0, 0, 0)):
            assert entry(bs, rates_of(zero), None) == entry(bs, None, None), zero
        assert entry(bs, rates_of(0.3), None) == entry(bs, rates_of((0, 0, 0.5)), None) == "camo_rg_loss_backward_drop"


@pytest.mark.parametrize("key", sorted(CONFIGS), ids=_key_id)
def test_configurations_stay_clear_of_a_relu_flip(key):
    c = _case(key)
    assert c["margin"] > DR.FLIP_MARGIN, (key, c["margin"])
    want = {0: {32, 33, 34, 35}, 1: {36}, 2: {37}}
    assert set(c["masks"]) == set().union(*(want[i] for i, v in enumerate(key[2]) if v > 0))


def test_the_configurations_are_the_issues():
    keys = set(CONFIGS)
    for mode in (0, 1):
        for rates in ((0.3, 0.0, 0.0), (0.0, 0.3, 0.0), (0.0, 0.0, 0.3), ALL):
            assert ("real", mode, rates) in keys
        for case in ("tail", "wide", "many"):
            assert (case, mode, ALL) in keys
    assert SHAPES["real"][1:4] == (23, 128, 4) and SHAPES["tail"][1] == 70 == 64 + 6 and SHAPES["wide"][1:3] == (9, 192)
    n = SHAPES["many"][1]
    c = _inputs("many", 1)
    assert n == c["x"].shape[0] > 1024 and -(-n // 64) == 17 and len(c["sizes"]) == 50
    assert not np.array_equal(c["mt"][:65], c["mt"][65:130])
    m = _case(("many", 1, ALL))["masks"]                                        # copies share weights, not masks
    assert not np.array_equal(m[33][:65], m[33][65:130]) and not np.array_equal(m[37][:65], m[37][65:130])


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def _direct(m, c, d, pair, mode, rates, seed):
    """camo_rg_loss_backward_drop called directly (the wrapper sends zero rates to the older entries): rg_train_calls.direct's record,
    every buffer having been between guard bands."""
    return direct("camo_rg_loss_backward_drop", m, d.x, pair, _targets(c), mode=mode, rates=rates, seed=seed, momentum=BR.MOMENTUM)


def _wrapper(m, c, d, pair, mode, rates, seed):
    """(loss [4], grads, batch_stats or None) through RegionGraphGNN.loss_and_gradients_csr"""
    bs = torch.full((4, 2, c["hidden"]), float("nan"), device="cuda") if mode else None
    loss, grads = m.loss_and_gradients_csr(d.x, *pair, *_targets(c), batch_stats=bool(mode), stats_out=bs, dropout=rates, seed=seed)
    return loss, grads, bs


def _same(a, b):
    return np.array_equal(_bits(a.detach().cpu()), _bits(b.detach().cpu()))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_zero_rates_are_the_existing_entry_byte_for_byte(mode):
    """N = 70 (64 + 6 rows), one CSR pair: losses, the 32 gradients, batch_stats and the updated running statistics of the new entry at
    rates 0 (whatever the seed) are the bytes of the mode's existing entry; the workspace queries are equal."""
    from camouflage_multimodal_amd import _lib
    c = _inputs("tail", mode)
    d = _data(c)
    pair = _csr_pair(c, d)
    old, new = _model(c).train(), _model(c).train()
    wl, wg, wbs = _wrapper(old, c, d, pair, mode, None, 0)
    got = _direct(new, c, d, pair, mode, (0.0, 0.0, 0.0), 0xDEADBEEF12345678)
    L, E = _lib.lib(), pair[0][1].shape[0]
    query = L.camo_rg_train_bn_workspace_bytes if mode else L.camo_rg_train_workspace_bytes
    assert got.need == query(ctypes.byref(old._dims), c["nc"], c["n"], E)
    assert _same(got.loss, wl)
    for k, a, b in zip(NAMES, got.grads, wg):
        assert _same(a, b), k
    if mode:
        assert _same(got.bs, wbs)
        want = _running(old)
        for k, a in zip(STAT_NAMES, got.run):
            assert np.array_equal(_bits(a.cpu()), _bits(want[k])) and not np.array_equal(_bits(want[k]), _bits(c["p"][k])), k
    # and the wrapper sends None, 0 and zeros down the existing entry
    for zero in (0, 0.0, (0, 0, 0)):
        l2, g2, _ = _wrapper(_model(c).train(), c, d, pair, mode, zero, 99)
        assert _same(l2, wl) and all(_same(a, b) for a, b in zip(g2, wg))


def _hold(c, loss4, grads, bs, running, tag):
    worst, worst32 = 0.0, 0.0

    def one(what, got, want64, want32):
        nonlocal worst, worst32
        e, e32 = _err(got, want64), _err(want32, want64)
        print(f"{tag} {what}: e {e:.3g} e32 {e32:.3g}")
        worst, worst32 = max(worst, e), max(worst32, e32)
        assert e <= _bound(e32), (tag, what, e, e32)

    for i, k in enumerate(LOSS_KEYS):
        one(k, loss4[i], c["l64"][i], c["l32"][i])
    for k in NAMES:
        assert grads[k].shape == c["g64"][k].shape, k
        if c["mode"] and k in BIAS_NAMES:
            assert not _bits(grads[k]).any(), (tag, k)                                     # every element is +0.0f, bit for bit
            continue
        one(k, grads[k], c["g64"][k], c["g32"][k])
    if c["mode"]:
        for k in range(4):
            for j, what in enumerate(("mean", "var")):
                one(f"batch {what} of bn{k + 1}", bs[k, j], c["bs64"][k, j], c["bs32"][k, j])
        for k in STAT_NAMES:
            one(k, running[k], c["run64"][k], c["run32"][k])
    print(f"{tag}: largest e {worst:.3g}, largest e32 {worst32:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(CONFIGS), ids=_key_id)
def test_gradients_and_statistics_match_float64(key):
    c = _case(key)
    assert c["margin"] > DR.FLIP_MARGIN                       # on the CPU reference, before the device is looked at
    m, d = _model(c).train(), _data(c)
    loss, grads, bs = _wrapper(m, c, d, _csr_pair(c, d), c["mode"], c["rates"], c["seed"])
    loss4 = loss.cpu().numpy().tolist()
    assert all(np.isfinite(v) for v in loss4), loss4
    _hold(c, loss4, {k: g.cpu().numpy() for k, g in zip(NAMES, grads)}, bs.cpu().numpy() if c["mode"] else None, _running(m), _key_id(key))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_same_seed_same_bytes_and_another_seed_another_loss(mode):
    c = _inputs("real", mode)
    d = _data(c)
    pair = _csr_pair(c, d)
    a = _wrapper(_model(c).train(), c, d, pair, mode, ALL, 5)
    b = _wrapper(_model(c).train(), c, d, pair, mode, ALL, 5)
    assert _same(a[0], b[0]) and all(_same(x, y) for x, y in zip(a[1], b[1])) and (not mode or _same(a[2], b[2]))
    other = _wrapper(_model(c).train(), c, d, pair, mode, ALL, 6)
    high = _wrapper(_model(c).train(), c, d, pair, mode, ALL, 5 + (1 << 32))       # the seed's high word is looked at
    assert not _same(a[0][:1], other[0][:1]) and not _same(a[0][:1], high[0][:1]) and not _same(other[0][:1], high[0][:1])
    assert all(bool(torch.isfinite(g).all()) for g in other[1] + high[1])


@pytest.mark.gpu
def test_head_dropout_alone_leaves_the_trunks_forward_alone():
    """p_head alone > 0: the trunk differs from the p = 0 call only through the backward, so the forward's batch_stats and the updated
    running statistics are the p = 0 call's bytes, while the loss and the trunk's gradients are not."""
    c = _inputs("real", 1)
    d = _data(c)
    pair = _csr_pair(c, d)
    m0, m1 = _model(c).train(), _model(c).train()
    l0, g0, b0 = _wrapper(m0, c, d, pair, 1, None, 0)
    l1, g1, b1 = _wrapper(m1, c, d, pair, 1, (0.0, 0.0, 0.3), 9)
    assert _same(b0, b1)
    r0, r1 = _running(m0), _running(m1)
    assert all(np.array_equal(_bits(r0[k]), _bits(r1[k])) for k in STAT_NAMES)
    assert not _same(l0[:1], l1[:1])
    for k, x, y in zip(NAMES, g0, g1):
        assert (k in BIAS_NAMES) == _same(x, y), k                              # (the conv biases: +0.0f in both)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_the_library_writes_inside_its_workspace_and_its_output_buffers(mode):
    """N = 70, called directly on a workspace of exactly the queried bytes and on output buffers of exactly their sizes, each between
    two 4 KiB sentinel bands: no guard byte changes, every output element is written, and the bytes are the wrapper's."""
    c = _inputs("tail", mode)
    d = _data(c)
    pair = _csr_pair(c, d)
    other = _model(c).train()
    wl, wg, wbs = _wrapper(other, c, d, pair, mode, ALL, 21)
    m = _model(c).train()
    got = _direct(m, c, d, pair, mode, ALL, 21)                 # (the guards and "every element written" are asserted there)
    outs = got.grads + [got.loss] + ([got.bs] + got.run if mode else [])
    refs = list(wg) + [wl] + ([wbs] + [other.state_dict()[k] for k in STAT_NAMES] if mode else [])
    names = NAMES + ["loss"] + (["batch_stats"] + list(STAT_NAMES) if mode else [])
    assert len(outs) == len(refs) == len(names)
    for k, val, ref in zip(names, outs, refs):
        assert _same(val, ref), k
    for k, v in m.state_dict().items():                       # the model whose tables were passed was not written
        assert torch.equal(v.cpu(), torch.from_numpy(c["p"][k].copy())) if k in c["p"] else int(v) == 0, k
