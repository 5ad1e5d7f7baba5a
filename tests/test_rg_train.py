"""Loss and gradients of the region-graph GNN with frozen batch-norm statistics (include/camo_rg_train.h) against
tests/rg_train_ref.py.

PARITY UNPINNED (the reference tree, torch_geometric and an RG checkpoint are absent): the header is the definition, the torch
restatement the checker.  CPU tests tie the restatement's logits to the two existing yardsticks (oracle/rg_gnn_oracle.py, then
tests/rg_detect_ref.py), its loss terms to torch's own, and the library's argument checks to the header.  GPU tests hold every one of
the 32 gradients and the four loss figures to float64 autograd:

    e = max|g - g64| / max(max|g64|, 1e-12)  <=  8 e32 + 2e-6,

e32 being the same error of torch-CPU float32 autograd of the same restatement, computed in the same test (8: another summation order;
2e-6: an e32 that is small by luck).  A gradient is discontinuous where a pre-activation crosses 0, so every case first asserts ON THE
CPU REFERENCE that no pre-activation (attention scores per edge, the four batch-norm outputs, the fc_shared output, the heads' hidden
layers) lies within 1e-4 max|tensor| of 0; the seeds below were found by a search on the CPU for that condition and are fixed.  No
element is ever left out of a comparison.

The case "real" (N = 23, hidden 128, heads 4, classes 2) prints its largest e and e32; DESIGN.md 9a records them.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import rg_detect_ref as R
import rg_train_ref as TR
from conftest import ROOT
from oracle import rg_gnn_oracle as RO

NAMES = TR.trainable_names()

# name: (graph kind, n, hidden, heads, classes, seed)
CASES = {
    "single": ("grid", 1, 128, 4, 2, 1),            # only the self-loop
    "isolated": ("isolated", 5, 128, 4, 2, 5),      # node 4 has no incoming edge but its self-loop
    "real": ("grid", 23, 128, 4, 2, 343),             # the real dimensions
    "tail": ("grid", 70, 32, 1, 3, 107),              # crosses 64 rows and the 4-nodes-per-block tail; half a wave idle
    "wide": ("grid", 23, 192, 2, 2, 3645),             # the CPL = 8 path
    "directed": ("directed", 12, 128, 4, 2, 110),     # no reverse edges, unequal weights, one explicit self-loop of weight 0.25
    "batch": ("batch", 64, 32, 2, 2, 11),            # 23 + 1 + 40 nodes at hidden 32, heads 2; some ignored targets
    "learn": ("grid", 23, 32, 4, 2, 15283),
}
BATCH_SIZES = (23, 1, 40)


def _graph(kind, n, seed):
    if kind == "grid":
        return RO.make_graph(n, seed)
    rs = np.random.RandomState(seed)
    x = rs.uniform(0, 1, size=(n, 15)).astype(np.float32)
    if kind == "isolated":
        pairs = [(0, 1), (1, 2), (2, 3), (0, 2)]
        src = [a for a, b in pairs] + [b for a, b in pairs] + [4]
        dst = [b for a, b in pairs] + [a for a, b in pairs] + [0]
        w = np.exp(-rs.uniform(0, 3, size=len(pairs))).astype(np.float32)
        return x, np.array([src, dst], np.int64), np.concatenate([w, w, [np.float32(0.6)]]).astype(np.float32)
    if kind == "directed":
        src = list(range(n)) + list(range(n)) + [3]
        dst = [(i + 1) % n for i in range(n)] + [(i + 5) % n for i in range(n)] + [3]
        w = np.exp(-rs.uniform(0, 3, size=2 * n)).astype(np.float32)
        assert not (set(zip(src, dst)) & set(zip(dst[:-1], src[:-1])))
        return x, np.array([src, dst], np.int64), np.concatenate([w, [np.float32(0.25)]]).astype(np.float32)
    assert kind == "batch" and n == sum(BATCH_SIZES)
    xs, eis, ews, off = [], [], [], 0
    for k, m in enumerate(BATCH_SIZES):
        gx, gei, gew = RO.make_graph(m, seed + 10 * k)
        xs.append(gx); eis.append(gei + off); ews.append(gew); off += m
    return np.concatenate(xs), np.concatenate(eis, 1), np.concatenate(ews)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and both CPU references of a case, computed once; never written to."""
    kind, n, hidden, heads, nc, seed = CASES[name]
    p = dict(RO.make_params(seed, 15, hidden, heads))
    p.update(R.make_head_params(seed + 1, hidden, nc))
    x, ei, ew = _graph(kind, n, seed)
    rs = np.random.RandomState(seed + 1000)
    mt = rs.randint(0, nc, size=n).astype(np.int32)
    it = rs.randint(0, nc, size=n).astype(np.int32)
    et = rs.uniform(0, 1, size=n).astype(np.float32)
    if kind == "batch":
        mt[[2, 23, 30]] = -1          # (23: the one-node graph has no mask target at all)
        et[[5, 40, 41, 63]] = -1.0
    l64, g64, margin = TR.loss_and_grads(p, x, ei, ew, mt, it, et, heads, nc)
    l32, g32, _ = TR.loss_and_grads(p, x, ei, ew, mt, it, et, heads, nc, dtype=torch.float32)
    for a in list(p.values()) + [x, ei, ew, mt, it, et]:
        a.setflags(write=False)
    return dict(p=p, x=x, ei=ei, ew=ew, mt=mt, it=it, et=et, l64=l64, g64=g64, margin=margin, l32=l32, g32=g32,
                hidden=hidden, heads=heads, nc=nc, n=n)


def _err(g, ref):
    g, ref = np.asarray(g, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(g - ref).max() / max(np.abs(ref).max(), 1e-12))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_restatement_logits_match_the_two_yardsticks():
    """The restatement's logits equal oracle/rg_gnn_oracle.node_embeddings followed by rg_detect_ref.heads to 1e-6 relative."""
    for name in ("real", "tail", "directed", "isolated"):
        c = _case(name)
        src, dst, w = RO.with_self_loops(c["n"], c["ei"], c["ew"])
        P = {k: torch.tensor(v, dtype=torch.float64) for k, v in c["p"].items()}
        taps = []
        logits = TR.forward(P, torch.tensor(c["x"], dtype=torch.float64), torch.tensor(src), torch.tensor(dst),
                            torch.tensor(w, dtype=torch.float64), c["heads"], taps).numpy()
        assert len(taps) == 9                                                            # s, bn1..4, fc_shared, three heads
        want = R.heads(c["p"], RO.node_embeddings(c["p"], c["x"], c["ei"], c["ew"], c["heads"]))
        e = np.abs(logits - want).max() / np.abs(want).max()
        print(name, "restatement against the yardsticks:", e)
        assert e <= 1e-6, (name, e)


def test_loss_terms_match_torch():
    F = torch.nn.functional
    l = torch.tensor([[0.3, -1.2, 2.0], [40.0, -40.0, 0.0], [-0.5, -0.5, -0.5], [1.0, 2.0, 3.0]], dtype=torch.float64)
    t = torch.tensor([2, -1, 0, 1])
    assert abs(float(TR.cross_entropy(l, t)) - float(F.cross_entropy(l, t, ignore_index=-1))) < 1e-12
    z = torch.tensor([0.0, 3.5, -60.0, 60.0, -2.0], dtype=torch.float64)
    y = torch.tensor([0.25, 1.0, 0.0, -1.0, 0.7], dtype=torch.float64)
    keep = y >= 0
    assert abs(float(TR.bce_with_logits(z, y)) - float(F.binary_cross_entropy_with_logits(z[keep], y[keep]))) < 1e-12
    logits = torch.cat([l[:, :2], l[:, 1:], z[:4, None]], 1)
    tot, lm, li, le = TR.losses(logits, torch.tensor([0, 1, -1, 1]), t.clamp(max=1), y[:4], (0.5, 2.0, 3.0), 2)
    assert abs(float(tot) - (0.5 * float(lm) + 2.0 * float(li) + 3.0 * float(le))) < 1e-12


def test_all_ignored_gives_zero_loss_and_zero_gradients():
    c = _case("isolated")
    n = c["n"]
    ls, g, _ = TR.loss_and_grads(c["p"], c["x"], c["ei"], c["ew"], np.full(n, -1, np.int32), np.full(n, -1, np.int32),
                                 np.full(n, -1.0, np.float32), c["heads"], c["nc"])
    assert ls == [0.0, 0.0, 0.0, 0.0]
    assert all(not np.any(g[k]) for k in NAMES)
    # one term alive: only its own head's second layer gets a gradient among the heads' second layers
    ls, g, _ = TR.loss_and_grads(c["p"], c["x"], c["ei"], c["ew"], np.full(n, -1, np.int32), c["it"], np.full(n, -1.0, np.float32),
                                 c["heads"], c["nc"])
    assert ls[1] == 0.0 and ls[3] == 0.0 and ls[0] == ls[2] > 0
    assert not np.any(g["fc_mask_2.weight"]) and not np.any(g["fc_edge_2.weight"]) and np.any(g["fc_instance_2.weight"])


def test_header_symbols_binding_and_abi_version():
    from camouflage_multimodal_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "camo_rg_train.h")).read()
    declared = set(re.findall(r"\b(camo_[a-z_0-9]+)\s*\(", hdr)) - {"camo_last_error"}
    assert declared == set(_lib.RGT_SYMBOLS), declared ^ set(_lib.RGT_SYMBOLS)
    assert "PARITY UNPINNED" in hdr and "train.py" in hdr
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared:
        assert hasattr(raw, s), s
    assert _lib.ABI_VERSION == 13 and "#define CAMO_ABI_VERSION 13" in open(os.path.join(ROOT, "include", "camo_fusion.h")).read()
    assert _lib.lib().camo_abi_version() == 13
    assert _lib.RGT_NGRADS == len(NAMES) == 32 and "CAMO_RGT_NGRADS = CAMO_RGT_HEADS + CAMO_RGD_NPARAMS" in hdr


def test_trainable_parameters_are_the_gradient_table():
    from camouflage_multimodal_amd import RegionGraphGNN
    m = RegionGraphGNN(hidden_channels=32, num_classes=3, heads=2)
    named = {id(p): k for k, p in m.named_parameters()}
    assert [named[id(p)] for p in m.trainable_parameters()] == NAMES
    assert len(list(m.parameters())) == 32


def test_argument_checks_match_the_header():
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()
    fake = 0x1000                                    # never dereferenced: every check runs on the host before any launch
    tabs = [(ctypes.c_void_p * n)(*([fake] * n)) for n in (28, 12, 32)]

    def call(hidden=128, nc=2, N=23, E=100, ws_bytes=None, null=None, heads=4, table_null=None):
        d = _lib.CamoRgDims(15, hidden, heads)
        need = L.camo_rg_train_workspace_bytes(ctypes.byref(d), nc, N, E)
        ptr = {k: fake for k in ("x", "rowptr", "col", "w", "rrowptr", "rcol", "rw", "mt", "it", "et", "ws", "loss")}
        t = list(tabs)
        if null in ptr:
            ptr[null] = None
        if null in ("params", "heads", "grads"):
            t[("params", "heads", "grads").index(null)] = None
        if table_null is not None:
            t[2] = (ctypes.c_void_p * 32)(*([fake] * 31 + [None]))
        rc = L.camo_rg_loss_backward(ctypes.byref(d), nc, t[0], t[1], ptr["x"], ptr["rowptr"], ptr["col"], ptr["w"], ptr["rrowptr"], ptr["rcol"],
                                     ptr["rw"], N, E, ptr["mt"], ptr["it"], ptr["et"], 1.0, 1.0, 1.0, ptr["ws"],
                                     need if ws_bytes is None else ws_bytes, ptr["loss"], t[2], None)
        return rc, need

    E_ARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3
    assert call(hidden=127) == (E_UNSUPPORTED, 0) and call(hidden=514) == (E_UNSUPPORTED, 0) and call(heads=9) == (E_UNSUPPORTED, 0)
    assert call(nc=1) == (E_UNSUPPORTED, 0) and call(nc=9) == (E_UNSUPPORTED, 0)
    assert call(N=0) == (E_UNSUPPORTED, 0) and call(N=23, E=22) == (E_UNSUPPORTED, 0)
    rc, need = call(ws_bytes=1024)
    assert rc == E_WORKSPACE and need > 1024
    assert call(ws_bytes=need - 1)[0] == E_WORKSPACE
    for name in ("x", "rowptr", "col", "w", "rrowptr", "rcol", "rw", "mt", "it", "et", "ws", "loss", "params", "heads", "grads"):
        assert call(null=name)[0] == E_ARG, name
    assert call(table_null=True)[0] == E_ARG
    assert b"gradient table" in L.camo_last_error()
    d = _lib.CamoRgDims(15, 128, 4)
    assert L.camo_rg_train_workspace_bytes(None, 2, 23, 100) == 0
    assert L.camo_rg_train_workspace_bytes(ctypes.byref(d), 2, 46, 200) > L.camo_rg_train_workspace_bytes(ctypes.byref(d), 2, 23, 100)


def test_cpu_tensors_raise():
    from camouflage_multimodal_amd import RegionGraphData, RegionGraphGNN
    from camouflage_multimodal_amd._lib import CamoError
    c = _case("isolated")
    m = RegionGraphGNN()
    data = RegionGraphData(torch.from_numpy(c["x"].copy()), torch.from_numpy(c["ei"].copy()), torch.from_numpy(c["ew"].copy())[:, None])
    with pytest.raises(CamoError):
        m.loss_and_gradients(data, torch.from_numpy(c["mt"].copy()), torch.from_numpy(c["it"].copy()), torch.from_numpy(c["et"].copy()))
    assert all(p.grad is None for p in m.parameters())


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_stay_clear_of_a_relu_flip(name):
    assert _case(name)["margin"] > TR.FLIP_MARGIN, (name, _case(name)["margin"])


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def _model(c):
    from camouflage_multimodal_amd import RegionGraphGNN
    m = RegionGraphGNN(hidden_channels=c["hidden"], num_classes=c["nc"], heads=c["heads"])
    sd = m.state_dict()
    for k, v in c["p"].items():
        assert tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.from_numpy(v.copy())
    m.load_state_dict(sd, strict=True)
    return m.cuda()


def _data(c, name=None):
    from camouflage_multimodal_amd import RegionGraphBatch, RegionGraphData
    x, ei, ea = torch.from_numpy(c["x"].copy()).cuda(), torch.from_numpy(c["ei"].copy()).cuda(), torch.from_numpy(c["ew"].copy()).cuda()[:, None]
    if name != "batch":
        return RegionGraphData(x, ei, ea)
    no = np.concatenate([[0], np.cumsum(BATCH_SIZES)])
    eo = [int((c["ei"][1] < b).sum()) for b in no]                 # (a graph's edges are contiguous and in graph order)
    batch = torch.from_numpy(np.repeat(np.arange(3), BATCH_SIZES).astype(np.int32)).cuda()
    return RegionGraphBatch(x, ei, ea, batch, [int(v) for v in no], eo)


def _embeddings_on_csr(m, x, csr):
    """extract_node_embeddings on a CSR the caller built (the public method builds its own, whose edge order within a row may differ
    from one build to the next): the same library call, so the same bytes for the same arrays."""
    from camouflage_multimodal_amd import _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    rowptr, col, w = csr
    n, L = x.shape[0], _lib.lib()
    ws = torch.empty(L.camo_rg_workspace_bytes(ctypes.byref(m._dims), n), dtype=torch.uint8, device=x.device)
    out = torch.empty(n, m._dims.hidden, dtype=torch.float32, device=x.device)
    tab, keep = m._param_table()
    _lib.check(L.camo_rg_node_embeddings(ctypes.byref(m._dims), tab, _ptr(x), _ptr(rowptr), _ptr(col), _ptr(w), n, col.shape[0], _ptr(ws),
                                         ws.numel(), _ptr(out), _stream_ptr()), "camo_rg_node_embeddings")
    return out


def _targets(c, sl=slice(None)):
    return tuple(torch.from_numpy(c[k][sl].copy()).cuda() for k in ("mt", "it", "et"))


def _device_grads(m):
    return {k: p.grad.detach().cpu().numpy() for k, p in zip(NAMES, m.trainable_parameters())}


def _hold(c, loss4, grads, tag):
    """Every loss figure and every gradient within 8 e32 + 2e-6 of float64; returns (largest e, largest e32)."""
    worst, worst32 = 0.0, 0.0
    for i, k in enumerate(("loss", "mask_loss", "instance_loss", "edge_loss")):
        e, e32 = _err(loss4[i], c["l64"][i]), _err(c["l32"][i], c["l64"][i])
        print(f"{tag} {k}: e {e:.3g} e32 {e32:.3g}")
        worst, worst32 = max(worst, e), max(worst32, e32)
        assert e <= 8 * e32 + 2e-6, (tag, k, e, e32)
    for k in NAMES:
        assert grads[k].shape == c["g64"][k].shape, k
        e, e32 = _err(grads[k], c["g64"][k]), _err(c["g32"][k], c["g64"][k])
        print(f"{tag} {k}: e {e:.3g} e32 {e32:.3g}")
        worst, worst32 = max(worst, e), max(worst32, e32)
        assert e <= 8 * e32 + 2e-6, (tag, k, e, e32)
    print(f"{tag}: largest e {worst:.3g}, largest e32 {worst32:.3g}")
    return worst, worst32


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["single", "isolated", "real", "tail", "wide", "directed", "batch"])
def test_gradients_match_float64_autograd(name):
    c = _case(name)
    assert c["margin"] > TR.FLIP_MARGIN                       # on the CPU reference, before the device is looked at
    m = _model(c).train()                                     # (whatever the mode: eval-mode arithmetic)
    out = m.loss_and_gradients(_data(c, name), *_targets(c))
    assert set(out) == {"loss", "mask_loss", "instance_loss", "edge_loss"} and all(v.dim() == 0 and v.is_cuda for v in out.values())
    _hold(c, [float(out[k]) for k in ("loss", "mask_loss", "instance_loss", "edge_loss")], _device_grads(m), name)


@pytest.mark.gpu
def test_two_calls_on_the_same_csr_give_the_same_bytes():
    from camouflage_multimodal_amd.region_graph import build_target_csr_device
    c = _case("real")
    m, d, t = _model(c).eval(), _data(c), _targets(c)
    csr = build_target_csr_device(c["n"], d.edge_index, d.edge_attr.reshape(-1))
    rcsr = build_target_csr_device(c["n"], d.edge_index.flip(0), d.edge_attr.reshape(-1))
    l1, g1 = m.loss_and_gradients_csr(d.x, csr, rcsr, *t)
    l2, g2 = m.loss_and_gradients_csr(d.x, csr, rcsr, *t)
    assert np.array_equal(_bits(l1.cpu()), _bits(l2.cpu()))
    for k, a, b in zip(NAMES, g1, g2):
        assert np.array_equal(_bits(a.cpu()), _bits(b.cpu())), k


@pytest.mark.gpu
def test_batch_is_the_count_weighted_sum_of_its_graphs():
    """Term t of the batch is a mean over cnt_t nodes, cnt_gt of them in graph g: d(batch) = sum_t sum_g cnt_gt / cnt_t d(term t of g)."""
    c = _case("batch")
    assert c["margin"] > TR.FLIP_MARGIN
    m, d = _model(c).eval(), _data(c, "batch")
    total = {k: np.zeros(c["g64"][k].shape) for k in NAMES}
    cnt = [int((c["mt"] >= 0).sum()), int((c["it"] >= 0).sum()), int((c["et"] >= 0).sum())]
    for g, graph in enumerate(d.graphs()):
        sl = slice(d.node_offsets[g], d.node_offsets[g + 1])
        for t in range(3):
            w = [0.0, 0.0, 0.0]
            w[t] = 1.0
            m.loss_and_gradients(graph, *_targets(c, sl), loss_weights=w)
            cg = int((c[("mt", "it", "et")[t]][sl] >= 0).sum())
            for k, v in _device_grads(m).items():
                total[k] += v.astype(np.float64) * (cg / cnt[t])
    for k in NAMES:
        e, e32 = _err(total[k], c["g64"][k]), _err(c["g32"][k], c["g64"][k])
        assert e <= 8 * e32 + 2e-6, (k, e, e32)


@pytest.mark.gpu
def test_accumulate_twice_is_twice_bit_for_bit_and_the_surface():
    c = _case("real")
    m, d, t = _model(c).eval(), _data(c), _targets(c)
    # one pair of CSRs for the whole test: the builder leaves a row's edges in no particular order, so two builds may add in two orders
    from camouflage_multimodal_amd.region_graph import build_target_csr_device
    pair = (build_target_csr_device(c["n"], d.edge_index, d.edge_attr.reshape(-1)),
            build_target_csr_device(c["n"], d.edge_index.flip(0), d.edge_attr.reshape(-1)))
    state = {k: v.clone() for k, v in m.state_dict().items()}
    emb0 = _embeddings_on_csr(m, d.x, pair[0])
    heads0 = m.node_heads(emb0)
    assert _err(m.extract_node_embeddings(d).cpu().numpy(), emb0.cpu().numpy()) <= 4e-5      # (the public call builds its own CSR; each is held to 2e-5 of float64)
    m.loss_and_gradients(d, *t)
    with_grad = [k for k, p in m.named_parameters() if p.grad is not None]
    assert sorted(with_grad) == sorted(NAMES) and len(with_grad) == 32
    for k, p in m.named_parameters():
        assert p.grad.shape == p.shape and p.grad.dtype == p.dtype and p.grad.is_cuda, k
    for k, v in m.state_dict().items():                       # running statistics and num_batches_tracked included
        assert torch.equal(v, state[k]), k
    emb1 = _embeddings_on_csr(m, d.x, pair[0])
    heads1 = m.node_heads(emb1)
    assert torch.equal(emb0, emb1) and torch.equal(heads0[0], heads1[0]) and torch.equal(heads0[1], heads1[1])
    m.loss_and_gradients(d, *t, csr=pair)
    once = {k: p.grad.clone() for k, p in m.named_parameters()}
    for p in m.parameters():
        p.grad.zero_()
    m.loss_and_gradients(d, *t, accumulate=True, csr=pair)
    m.loss_and_gradients(d, *t, accumulate=True, csr=pair)
    for k, p in m.named_parameters():                         # (exact equality of every element; 0 + -0 + -0 is +0 where 2 * -0 is -0)
        assert torch.equal(p.grad, 2 * once[k]) and bool(torch.isfinite(p.grad).all()), k
    m.loss_and_gradients(d, *t, csr=pair)                       # without accumulate: set, not added
    for k, p in m.named_parameters():
        assert np.array_equal(_bits(p.grad.cpu()), _bits(once[k].cpu())), k


@pytest.mark.gpu
def test_it_learns_and_follows_the_float64_steps():
    c = _case("learn")
    lr, steps = 0.05, 10
    # the reference alone: decreases, and stays clear of a flip at every step
    p = {k: v.astype(np.float64) for k, v in c["p"].items()}
    ref = []
    for _ in range(steps + 1):
        ls, g, margin = TR.loss_and_grads(p, c["x"], c["ei"], c["ew"], c["mt"], c["it"], c["et"], c["heads"], c["nc"])
        assert margin > TR.FLIP_MARGIN, margin
        ref.append(ls[0])
        for k in NAMES:
            p[k] = p[k] - lr * g[k]
    assert ref[steps] < ref[0]
    m, d, t = _model(c).train(), _data(c), _targets(c)
    opt = torch.optim.SGD(m.trainable_parameters(), lr=lr)
    got = []
    for _ in range(steps + 1):
        got.append(float(m.loss_and_gradients(d, *t)["loss"]))
        opt.step()
    print("reference", ref[0], ref[steps], "device", got[0], got[steps])
    assert got[steps] < got[0]
    assert abs(got[steps] - ref[steps]) <= 1e-3 * abs(ref[steps])
