"""The region-graph INFERENCE forward (camo_rg_node_embeddings: gat_aggregate_kernel's online softmax with __expf, the non-saving
gcn_aggregate_kernel; camo_rg_build_csr; camo_rg_node_heads) against float64, off the tame graphs.

tests/test_rg_gnn.py holds that path to the fp32 numpy oracle on RO.make_graph graphs only: symmetric, at most about 6 entries per row,
parameters at initialisation scale.  On such a graph an inference path that reads edge_index the wrong way round, drops a repeated edge
or ignores a self-loop's weight computes the same numbers (the blindness table below, reproduced by a CPU test).  The training forward
has kernels of its own (csrc/rg_abi.hip: "Two GAT kernels on purpose"), so tests/test_rg_train.py's hard cases never reach these.

PARITY UNPINNED: the header and the tests are the definition.  The reference is relu of the sixth tap (the fc_shared pre-activation) of
tests/rg_train_ref.forward in float64 on the fp32 inputs, with the edge list of RO.with_self_loops; a CPU test ties it to
oracle/rg_gnn_oracle.node_embeddings at 1e-6.  e32 is the same forward in torch float32: the cost of fp32 arithmetic alone.  All figures
are max|got - ref64| / max|ref64|, and the device is held to the project's own bound, |got - ref64| <= 2e-5 max|ref64| + 2e-6
(tests/test_rg_gnn.py, tests/test_rg_detect.py; rg_train_ref.FLIP_MARGIN rests on it).  Every case first asserts ON THE REFERENCE what
it claims to exercise, e32 <= 1e-6 among it, so the bound sits at least 20 x above fp32 noise.

max|d emb| / max|emb| of the float64 reference when its edge list is corrupted before the forward:

    corruption of the edge list                a make_graph case    hub301    directed-real
    repeated edges dropped                     0 exactly            1.6e-2    0
    explicit self-loop weight replaced by 1    0 exactly            0         2.1e-1
    source and target exchanged                0 exactly            1.6e-2    1.7e-1

Measured on an MI355X, the public call (device-built CSR, whose order within a row moves from build to build) and the host-built
sorted CSR together; e32 between 1.4e-7 and 5.6e-7 throughout (it moves with the host's BLAS), the bound at 2e-5:

    case group                                              worst e     worst e / e32
    isolated, directed, sharp, steep, hub, single, many     3.9e-7      1.66 ("single")
    hub301, hub301-sharp, hub301-steep                      3.2e-7      1.20
    directed-real, zero-degree                              2.0e-7      0.63
    widest, w130, w129, in33, in1                           4.3e-7      1.00
    hub301-sharp, -steep with rows by ascending and by
    descending score                                        5.0e-7      1.58

and e 3.7e-7 on the block-diagonal batch, 4.0e-7 on the unweighted graphs; the saturated heads' logits within 9.7e-7 (absolute, at
max|logit| 30.1) and their probabilities within 4.3e-11.

No kernel needed a change: the inference forward is where fp32 arithmetic puts it on all of these.  Mutation check (scratch builds,
not committed): camo_rg_build_csr reading edge_index the wrong way round fails 12 of this file's GPU tests ("isolated", "directed",
"hub", the hub301 family, "directed-real", "zero-degree", the batch, both unweighted cases, the builder's extents on "hub"); a
csr_count_kernel / csr_fill_kernel that skip an edge already seen fail 7 ("hub", the hub301 family, the batch, unweighted hub301, the
builder's extents on "hub"); tests/test_rg_gnn.py's 14 GPU tests pass on both.  (A csr_count_kernel that gives an explicit self-loop
weight 1 fails 4 here -- "directed", "directed-real", "zero-degree", the batch -- and was already seen by test_rg_gnn.py's builder
test, which appends such a loop, though by none of its embedding tests.)
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import rg_detect_ref as R
import rg_train_ref as TR
from oracle import rg_gnn_oracle as RO
from guarded import guarded as _guarded, guards_intact as _guards_intact
from test_rg_train import _case, _data, _embeddings_on_csr, _graph, _model, _saturate, _sharpen

REUSED = ("isolated", "directed", "sharp", "steep", "hub", "single", "many")       # of test_rg_train.CASES, through _case
# name: (graph kind, n, in_channels, hidden, heads, seed, (att_src gain, att_dst gain) or None)
NEW = {
    "hub301": ("hub", 301, 15, 128, 4, 7, None),                   # row 0 has 302 entries; 1 -> 0 and 0 -> 2 listed twice
    "hub301-sharp": ("hub", 301, 15, 128, 4, 7, (20, 20)),         # max|s| 46.8; row 0's largest alpha per head 0.94 / 0.80 / 0.07 / 0.67
    "hub301-steep": ("hub", 301, 15, 128, 4, 7, (20, -20)),        # top score 62.4
    "directed-real": ("directed", 12, 15, 128, 4, 110, None),      # one-way edges, an explicit self-loop of weight 0.25
    "zero-degree": ("directed", 12, 15, 128, 4, 3, None),          # the graph of seed 110 with deg[2] = 0 (see _inputs)
    "widest": ("grid", 9, 15, 512, 8, 8, None),                    # both launch limits at once: 512 threads and 16 KB of LDS, CPL = 8 full
    "w130": ("grid", 70, 15, 130, 3, 9, None),                     # the first even width past the 128 switch, no multiple of 64; the 4-nodes-per-block tail
    "w129": ("grid", 23, 15, 129, 2, 9, None),                     # an odd width (embeddings only: the heads need an even one)
    "in33": ("grid", 23, 33, 64, 8, 10, None),
    "in1": ("grid", 23, 1, 32, 1, 10, None),
}
ALL = REUSED + tuple(NEW)
GRIDS = ("sharp", "steep", "single") + tuple(k for k, v in NEW.items() if v[0] == "grid")       # the make_graph cases
LN_FLT_MAX = float(np.log(np.finfo(np.float32).max))               # 88.72


def _inputs(name):
    kind, n, cin, hidden, heads, seed, gains = NEW[name]
    p = dict(RO.make_params(seed, cin, hidden, heads))
    p.update(R.make_head_params(seed + 1, hidden, 2))
    if gains:
        _sharpen(p, *gains)
    if name == "zero-degree":
        x, ei, ew = _graph(kind, n, 110)
        ew = ew.copy()
        ew[ei[1] == 2] = 0.0                                       # (the graph's one explicit self-loop is 3 -> 3)
        ei, ew = np.concatenate([ei, [[2], [2]]], 1), np.concatenate([ew, [np.float32(0)]]).astype(np.float32)
    elif kind == "grid":
        x, ei, ew = RO.make_graph(n, seed, cin)
    else:
        x, ei, ew = _graph(kind, n, seed)
    return dict(p=p, x=x, ei=ei, ew=ew, hidden=hidden, heads=heads, nc=2, n=n, sizes=None)


def _embeddings(p, x, heads, edges, dtype=torch.float64):
    """relu of the sixth tap of the restatement's forward on the edge list `edges` = (src, dst, w), self-loops included."""
    src, dst, w = edges
    P = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in p.items()}
    taps = []
    TR.forward(P, torch.tensor(x, dtype=dtype), torch.tensor(src), torch.tensor(dst), torch.tensor(w, dtype=dtype), heads, taps)
    assert len(taps) == 9                                          # s, bn1..4, fc_shared, three heads
    return torch.relu(taps[5]).numpy().astype(np.float64)


def _edges(c, ew="own"):
    return RO.with_self_loops(c["n"], c["ei"], c["ew"] if isinstance(ew, str) else ew)


def _rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def _bound(ref):
    return 2e-5 * float(np.abs(ref).max()) + 2e-6


@functools.lru_cache(maxsize=None)
def _c(name):
    """Inputs and both CPU references of a case, computed once; never written to."""
    c = dict(_case(name)) if name in REUSED else _inputs(name)
    c["in_channels"] = c["x"].shape[1]
    c["ref64"] = _embeddings(c["p"], c["x"], c["heads"], _edges(c))
    c["e32"] = _rel(_embeddings(c["p"], c["x"], c["heads"], _edges(c), torch.float32), c["ref64"])
    for a in list(c["p"].values()) + [c["x"], c["ei"], c["ew"], c["ref64"]]:
        a.setflags(write=False)
    return c


def _scores(c):
    """(src, dst, s [E', heads]) in float64: the attention scores a_src[j] + a_dst[i] of every edge j -> i, before the leaky ReLU."""
    src, dst, _ = _edges(c)
    n, heads, hidden = c["n"], c["heads"], c["hidden"]
    f = lambda k: c["p"][k].astype(np.float64)  # noqa: E731
    h = (c["x"].astype(np.float64) @ f("conv1.lin.weight").T).reshape(n, heads, hidden)
    a_src, a_dst = (h * f("conv1.att_src").reshape(1, heads, hidden)).sum(-1), (h * f("conv1.att_dst").reshape(1, heads, hidden)).sum(-1)
    return src, dst, a_src[src] + a_dst[dst]


def _lrelu(s):
    return np.where(s > 0, s, 0.2 * s)


# ---- CPU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_restatement_matches_the_oracle_and_the_case_is_what_it_claims(name):
    """On the reference alone, before any device is looked at."""
    c = _c(name)
    ref = c["ref64"]
    e = _rel(RO.node_embeddings(c["p"], c["x"], c["ei"], c["ew"], c["heads"]), ref)
    nonzero = float((ref != 0).mean())
    print(f"{name}: restatement against the oracle {e:.3g}, e32 {c['e32']:.3g}, non-zero {nonzero:.2f}")
    assert ref.shape == (c["n"], c["hidden"]) and c["x"].shape == (c["n"], c["in_channels"])
    assert e <= 1e-6, (name, e)
    assert c["e32"] <= 1e-6, (name, c["e32"])
    assert np.isfinite(ref).all() and 0.25 <= nonzero <= 0.75, (name, nonzero)


def test_the_new_cases_are_where_they_claim_to_be():
    h = _c("hub301")
    src, dst, _ = _edges(h)
    pairs = list(zip(src.tolist(), dst.tolist()))
    assert int((dst == 0).sum()) == 302 and len(pairs) - len(set(pairs)) == 2 and pairs.count((1, 0)) == 2 and pairs.count((0, 2)) == 2
    for k in ("hub301-sharp", "hub301-steep"):                    # the same graph and features
        assert all(np.array_equal(_c(k)[a], h[a]) for a in ("x", "ei", "ew"))
    src, dst, s = _scores(_c("hub301-sharp"))
    e0 = _lrelu(s[dst == 0])
    alpha = np.exp(e0 - e0.max(0)) / np.exp(e0 - e0.max(0)).sum(0)
    print("hub301-sharp: max|s|", np.abs(s).max(), "row 0's largest alpha per head", alpha.max(0))
    assert np.abs(s).max() > 40 and alpha.max(0).max() > 0.9 and alpha.max(0).min() < 0.1
    top = {k: float(_scores(_c(k))[2].max()) for k in ("hub301-steep", "steep")}
    print("top scores", top)
    # only "steep" crosses ln FLT_MAX; hub301-steep reaches 62.4 (measured), where the online softmax's corrections are large, not infinite
    assert top["steep"] > LN_FLT_MAX > top["hub301-steep"] > 60
    z = _c("zero-degree")
    src, dst, w = _edges(z)
    assert float(w[dst == 2].sum()) == 0.0 and int((dst == 2).sum()) == 3 and (w[dst != 2] > 0).all()       # deg[2] == 0, and only there
    assert w[(src == 2) & (dst == 2)].tolist() == [0.0] and int(((src == 2) & (dst != 2)).sum()) == 2       # node 2 still feeds two others
    d = _c("directed-real")
    src, dst, w = _edges(d)
    one_way = set(zip(src[src != dst].tolist(), dst[src != dst].tolist()))
    assert len(one_way) == 24 and not (one_way & {(b, a) for a, b in one_way}) and w[(src == 3) & (dst == 3)].tolist() == [0.25]
    assert (_c("widest")["hidden"], _c("widest")["heads"]) == (512, 8) and _c("w130")["n"] % 4 == 2 and _c("w130")["n"] > 64


def _corrupt(edges, how):
    src, dst, w = (a.copy() for a in edges)
    if how == "repeated edges dropped":
        _, first = np.unique(np.stack([src, dst]), axis=1, return_index=True)
        keep = np.sort(first)
        src, dst, w = src[keep], dst[keep], w[keep]
    elif how == "self-loop weight replaced by 1":
        w[src == dst] = 1.0
    else:
        assert how == "source and target exchanged"
        src, dst = dst, src
    order = np.lexsort((src, dst))                                 # (the order RO.with_self_loops gives: one summation order for all)
    return src[order], dst[order], w[order]


CORRUPTIONS = ("repeated edges dropped", "self-loop weight replaced by 1", "source and target exchanged")


def _blindness(name, how):
    c = _c(name)
    return _rel(_embeddings(c["p"], c["x"], c["heads"], _corrupt(_edges(c), how)), c["ref64"])


def test_blindness_table():
    """What a make_graph graph cannot see, and which case sees it: each corruption of the reference's edge list is exactly 0 on every
    make_graph case and at least 100 x the device bound (2e-3) on the case named for it."""
    for name in GRIDS:
        for how in CORRUPTIONS:
            assert _blindness(name, how) == 0.0, (name, how)
    table = {(name, how): _blindness(name, how) for name in ("hub301", "directed-real") for how in CORRUPTIONS}
    for k, v in table.items():
        print(k, f"{v:.3g}")
    assert table["hub301", CORRUPTIONS[0]] >= 2e-3 and table["directed-real", CORRUPTIONS[0]] == 0.0
    assert table["directed-real", CORRUPTIONS[1]] >= 2e-3 and table["hub301", CORRUPTIONS[1]] == 0.0
    assert table["directed-real", CORRUPTIONS[2]] >= 2e-3 and table["hub301", CORRUPTIONS[2]] >= 2e-3
    # the fourth: a GAT softmax without its row maximum, in float32
    def unshifted(name):
        src, dst, s = _scores(_c(name))
        with np.errstate(over="ignore", invalid="ignore"):
            p = np.exp(_lrelu(s).astype(np.float32))
            den = np.zeros((_c(name)["n"], s.shape[1]), np.float32)
            np.add.at(den, dst, p)
            return p / den[dst]
    assert np.isfinite(unshifted("w130")).all() and not np.isfinite(unshifted("steep")).all()


def test_grid_cases_are_the_make_graph_cases():
    assert set(GRIDS) == {"sharp", "steep", "single", "widest", "w130", "w129", "in33", "in1"}
    for name in GRIDS:
        c = _c(name)
        pairs = dict(zip(zip(c["ei"][0].tolist(), c["ei"][1].tolist()), c["ew"].tolist()))
        assert len(pairs) == c["ei"].shape[1] and all(pairs[(b, a)] == v and a != b for (a, b), v in pairs.items())       # symmetric, no repeats, no loops


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def _gnn(c):
    if c["in_channels"] == 15:
        return _model(c).eval()
    from camouflage_multimodal_amd import RegionGraphGNN
    m = RegionGraphGNN(in_channels=c["in_channels"], hidden_channels=c["hidden"], num_classes=c["nc"], heads=c["heads"])
    sd = m.state_dict()
    for k, v in c["p"].items():
        assert tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.from_numpy(v.copy())
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def _host_csr(c, ew="own"):
    from camouflage_multimodal_amd import build_target_csr
    ew = c["ew"] if isinstance(ew, str) else ew
    return build_target_csr(c["n"], torch.from_numpy(c["ei"].copy()), None if ew is None else torch.from_numpy(ew.copy()))


def _held(got, ref, tag, e32=None):
    """Shape, finiteness and the project's bound against float64; returns e."""
    got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float32, (tag, got.shape)
    assert np.isfinite(got).all(), tag
    err, e = float(np.abs(got - ref).max()), _rel(got, ref)
    print(f"{tag}: e {e:.3g}" + ("" if e32 is None else f" e32 {e32:.3g} e / e32 {e / e32:.3g}") + f" (max error {err:.3g}, bound {_bound(ref):.3g})")
    assert err <= _bound(ref), (tag, err, _bound(ref))
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_inference_embeddings_match_float64(name):
    c = _c(name)
    assert c["e32"] <= 1e-6                                       # on the CPU reference, before the device is looked at
    m, d = _gnn(c), _data(c)
    _held(m.extract_node_embeddings(d), c["ref64"], f"{name} (public call, device-built CSR)", c["e32"])
    _held(_embeddings_on_csr(m, d.x, [t.cuda() for t in _host_csr(c)]), c["ref64"], f"{name} (host-built sorted CSR)", c["e32"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hub301-sharp", "hub301-steep"])
def test_row_order_does_not_move_the_online_softmax(name):
    """Every row of the host CSR with its self-loop first and the rest by ascending head-0 score lrelu(a_src[j] + a_dst[i]) of the
    float64 reference -- every edge raises the online softmax's running maximum, and the sum so far is scaled down 300 times in row 0 --
    and by descending score, where none does."""
    c = _c(name)
    rowptr, col, w = [t.numpy() for t in _host_csr(c)]
    src, dst, s = _scores(c)
    assert np.array_equal(col, src) and np.array_equal(rowptr, np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=c["n"]))]))
    score = _lrelu(s[:, 0])
    m, x = _gnn(c), torch.from_numpy(c["x"].copy()).cuda()
    got = {}
    for sign in (1.0, -1.0):
        loop = (src == dst).astype(np.int64)
        order = np.lexsort((sign * score, 1 - loop, dst))          # by row; the self-loop, then by the score
        assert np.array_equal(dst[order], dst)
        for i in range(c["n"]):
            assert col[order][rowptr[i]] == i and (np.diff(sign * score[order][rowptr[i] + 1:rowptr[i + 1]]) >= 0).all(), i
        assert int((np.diff(sign * score[order][1:rowptr[1]]) > 0).sum()) >= 299      # row 0: (nearly) every edge moves the maximum, or none
        csr = (torch.from_numpy(rowptr).cuda(), torch.from_numpy(col[order].copy()).cuda(), torch.from_numpy(w[order].copy()).cuda())
        got[sign] = _embeddings_on_csr(m, x, csr)
        _held(got[sign], c["ref64"], f"{name} ({'ascending' if sign > 0 else 'descending'} scores)", c["e32"])
    assert float((got[1.0] - got[-1.0]).abs().max()) <= 2 * _bound(c["ref64"])


@pytest.mark.gpu
def test_block_diagonal_batch_matches_the_float64_reference_of_each_graph():
    """hub301-steep, the one-node graph of "single" and directed-real as one graph with offset indices, on hub301-steep's parameters:
    each graph's rows against ITS float64 reference (not device against device)."""
    from camouflage_multimodal_amd import RegionGraphData
    a, parts = _c("hub301-steep"), [_c("hub301-steep"), _c("single"), _c("directed-real")]
    assert all((g["hidden"], g["heads"], g["in_channels"]) == (128, 4, 15) for g in parts) and parts[1]["n"] == 1
    refs = [a["ref64"]] + [_embeddings(a["p"], g["x"], 4, _edges(g)) for g in parts[1:]]
    off = np.concatenate([[0], np.cumsum([g["n"] for g in parts])])
    x = torch.from_numpy(np.concatenate([g["x"] for g in parts])).cuda()
    ei = torch.from_numpy(np.concatenate([g["ei"] + off[k] for k, g in enumerate(parts)], 1)).cuda()
    ea = torch.from_numpy(np.concatenate([g["ew"] for g in parts])).cuda()[:, None]
    got = _gnn(a).extract_node_embeddings(RegionGraphData(x, ei, ea))
    assert got.shape == (int(off[-1]), 128)
    for k, g in enumerate(parts):
        _held(got[off[k]:off[k + 1]], refs[k], f"batch, graph {k} ({g['n']} nodes)")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["directed-real", "hub301"])
def test_unweighted_graphs_match_float64_with_unit_weights(name):
    """edge_attr=None and an edge_attr without elements: every weight 1, an explicit self-loop's too."""
    c = _c(name)
    ref = _embeddings(c["p"], c["x"], c["heads"], _edges(c, None))
    assert _rel(ref, c["ref64"]) > 2e-3                            # (the weights matter on this graph)
    m, d = _gnn(c), _data(c)
    _held(m.extract_node_embeddings(x=d.x, edge_index=d.edge_index, edge_attr=None), ref, f"{name} (edge_attr=None)")
    _held(m.extract_node_embeddings(x=d.x, edge_index=d.edge_index, edge_attr=torch.zeros(0, 1).cuda()), ref, f"{name} (empty edge_attr)")
    _held(_embeddings_on_csr(m, d.x, [t.cuda() for t in _host_csr(c, None)]), ref, f"{name} (host-built CSR, no weights)")


def _bits(t):
    return t.contiguous().view(torch.uint8).reshape(-1).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["widest", "hub301", "many"])
def test_node_embeddings_write_inside_their_workspace_and_their_output(name):
    """camo_rg_node_embeddings called directly on a workspace of exactly camo_rg_workspace_bytes and an output of exactly n hidden
    floats, each a 256-byte-aligned piece in the middle of a sentinel-filled tensor this test owns: no byte outside a declared extent
    changes, every output element is written (the output's sentinel 0xFF is a NaN), and the bytes are those of _embeddings_on_csr on
    the same arrays.  Nothing is overrun: a stray write would land in memory this test owns, where it is seen."""
    from camouflage_multimodal_amd import _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    from camouflage_multimodal_amd.region_graph import build_target_csr_device
    c = _c(name)
    m, d = _gnn(c), _data(c)
    n, L = c["n"], _lib.lib()
    x = d.x.contiguous()
    rowptr, col, w = build_target_csr_device(n, d.edge_index, d.edge_attr.reshape(-1))
    want = _embeddings_on_csr(m, x, (rowptr, col, w))
    need = L.camo_rg_workspace_bytes(ctypes.byref(m._dims), n)
    assert need > 0
    ws_whole, ws = _guarded(need, 0xA5)
    out_whole, out = _guarded(4 * n * c["hidden"], 0xFF)
    assert bool(torch.isnan(out.view(torch.float32)).all())
    tab, keep = m._param_table()
    _lib.check(L.camo_rg_node_embeddings(ctypes.byref(m._dims), tab, _ptr(x), _ptr(rowptr), _ptr(col), _ptr(w), n, col.shape[0], _ptr(ws), need,
                                         _ptr(out), _stream_ptr()), "camo_rg_node_embeddings")
    torch.cuda.synchronize()
    assert _guards_intact(ws_whole, ws, 0xA5), "workspace"
    assert _guards_intact(out_whole, out, 0xFF), "out"
    assert bool(torch.isfinite(out.view(torch.float32)).all())    # every element written: none is the sentinel any more
    assert np.array_equal(_bits(out), _bits(want))
    assert L.camo_rg_node_embeddings(ctypes.byref(m._dims), tab, _ptr(x), _ptr(rowptr), _ptr(col), _ptr(w), n, col.shape[0], _ptr(ws), need - 1,
                                     _ptr(out), _stream_ptr()) == -3           # CAMO_E_WORKSPACE: one byte less is refused before any launch


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hub", "many"])
def test_csr_builder_writes_inside_its_extents(name):
    """camo_rg_build_csr on buffers of exactly the sizes build_target_csr_device gives them (scratch 3 N int32, rowptr N + 1, col and w
    E + N), each inside a guarded tensor: guards intact, rowptr the host builder's, every row the host builder's as a multiset with the
    self-loop first (so every element of rowptr, col and w is written)."""
    from camouflage_multimodal_amd import _lib, build_target_csr
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    c = _c(name)
    n, E, L = c["n"], c["ei"].shape[1], _lib.lib()
    ei, ew = torch.from_numpy(c["ei"].copy()).cuda().contiguous(), torch.from_numpy(c["ew"].copy()).cuda().contiguous()
    assert ei.dtype == torch.int64 and ew.dtype == torch.float32
    bufs = {k: _guarded(4 * k_n, 0xA5) for k, k_n in (("scratch", 3 * n), ("rowptr", n + 1), ("col", E + n), ("w", E + n))}
    _lib.check(L.camo_rg_build_csr(_ptr(ei), _ptr(ew), n, E, *[_ptr(bufs[k][1]) for k in ("scratch", "rowptr", "col", "w")], _stream_ptr()),
               "camo_rg_build_csr")
    torch.cuda.synchronize()
    for k, (whole, piece) in bufs.items():
        assert _guards_intact(whole, piece, 0xA5), k
    r1, c1 = (bufs[k][1].view(torch.int32).cpu().numpy() for k in ("rowptr", "col"))
    w1 = bufs["w"][1].view(torch.float32).cpu().numpy()
    r0, c0, w0 = [t.numpy() for t in build_target_csr(n, torch.from_numpy(c["ei"].copy()), torch.from_numpy(c["ew"].copy()))]
    assert np.array_equal(r0, r1) and r1[n] == E + n
    for i in range(n):
        assert sorted(zip(c0[r0[i]:r0[i + 1]].tolist(), w0[r0[i]:r0[i + 1]].tolist())) == \
            sorted(zip(c1[r1[i]:r1[i + 1]].tolist(), w1[r1[i]:r1[i + 1]].tolist())), i
        assert c1[r1[i]] == i                                      # the self-loop leads its row


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,nc,n", [(128, 2, 17), (384, 3, 9)])          # one row past a tile of 16; one past the other tile of 8
def test_node_heads_write_inside_their_outputs(hidden, nc, n):
    from camouflage_multimodal_amd import RegionGraphGNN, _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    torch.manual_seed(hidden)
    m = RegionGraphGNN(hidden_channels=hidden, num_classes=nc).cuda().eval()
    emb = torch.from_numpy(np.maximum(np.random.RandomState(n).standard_normal((n, hidden)), 0).astype(np.float32)).cuda()
    want = m.node_heads(emb)
    outs = [_guarded(4 * n * (2 * nc + 1), 0xFF), _guarded(4 * n * 3, 0xFF)]
    htab, keep = m._head_table()
    _lib.check(_lib.lib().camo_rg_node_heads(ctypes.byref(m._dims), nc, htab, _ptr(emb), n, _ptr(outs[0][1]), _ptr(outs[1][1]), _stream_ptr()),
               "camo_rg_node_heads")
    torch.cuda.synchronize()
    for (whole, piece), ref, k in zip(outs, want, ("logits", "probs")):
        assert _guards_intact(whole, piece, 0xFF), k
        assert bool(torch.isfinite(piece.view(torch.float32)).all()), k          # everything written
        assert np.array_equal(_bits(piece), _bits(ref)), k


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1, -1])
def test_saturated_heads_at_inference(sign):
    """The inference heads kernel (__expf softmax and sigmoid) at last-layer biases of +-25, -+12 and 30, and with them negated (the
    sigmoid's __expf argument large and positive), on the float64 reference embeddings of hub301 cast to fp32 -- no GNN kernel runs."""
    c = _c("hub301")
    p = dict(c["p"])
    _saturate(p)
    for k in ("fc_mask_2.bias", "fc_instance_2.bias", "fc_edge_2.bias"):
        p[k] = (sign * p[k]).astype(np.float32)
    emb = c["ref64"].astype(np.float32)
    want = R.heads(p, emb)
    wantp = R.probabilities(want, 2)
    assert float(np.abs(want).max()) > 20 and float((sign * want[:, 4]).min()) > 20       # on the reference, first
    logits, probs = _model(dict(c, p=p)).eval().node_heads(torch.from_numpy(emb).cuda())
    logits, probs = logits.cpu().numpy(), probs.cpu().numpy()
    bound = 2e-5 * float(np.abs(want).max()) + 2e-6
    el, ep = float(np.abs(logits - want).max()), float(np.abs(probs - wantp).max())
    print(f"biases x {sign}: max |logits - float64| = {el:.3e} (bound {bound:.3e}), max |probs - float64| = {ep:.3e} "
          f"(bound {bound / 2 + 2e-6:.3e}), max |ref| = {float(np.abs(want).max()):.3f}")
    assert logits.shape == (301, 5) and probs.shape == (301, 3)
    assert np.isfinite(logits).all() and np.isfinite(probs).all() and probs.min() >= 0.0 and probs.max() <= 1.0
    assert el <= bound
    assert ep <= bound / 2 + 2e-6
