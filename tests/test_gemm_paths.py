"""The grouped GEMM (csrc/gemm.hip) on every path its launcher and kernels pick from the arguments alone, against exact integers.

Exact by construction: A and B hold integers in [-3, 3] (exact in bf16 too), bias, residual and the initial C and bias_grad integers in
[-64, 64], and aux_scale, 1 / uniform_n, inv_nr and the dropout scale (p = 0.5) are powers of two.  Every product, every partial sum in
any order and every atomic add is then an integer (or a dyadic fraction) below 2**24 in magnitude, which fp32 holds exactly: the
reference is an int64 product with a float64 epilogue and the comparison is BYTEWISE in both precisions, over the whole of every output
array, pad columns included.  Each case asserts that precondition on the CPU first.

``path`` restates the launcher's arithmetic (kernel, PIPE, ksplit, kchunk, VEC, v4 or scalar epilogue).  Every case asserts the path it
was written for, and CPU tests assert that the case list has both sides of every rule, so the suite shows its coverage without a GPU.

The two kernels, and a split and an unsplit K loop, give the same bytes on such data.  Which kernel ran is read from the library's launch
timing around every case (camo_prof_kind), and the split-K threshold from one case that leaves the exact range on purpose (2**24 + 1 + 1).

Three comparisons are not bytewise:
  * GF_SIGMOID: pre-activations are integers in [-6, 6] (a unit error moves the result by >= 2.4e-3); compared with float64 at
    SIGMOID_TOL = 1.98e-7 = 4 x the worst error measured on an MI355X over these cases (4.944e-8, under one ulp below 1).
  * GF_RES_BCAST with uniform_n = 3: 2**-23 (|v| + |res / 3|), one rounding of the quotient and one of the sum, fused or not.
  * the bf16 rounding mode (integers cannot see it): real operands at prec = 1 against the float64 product of the oracle's RNE-rounded
    operands at tests/test_hip_gemm16.py's bound, 2e-6 (|a| @ |b| + 1); measured on an MI355X: at most 0.048 of that bound.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle.fusion_oracle import bf16_round, dropout_keep
from raw_calls import execute, gemm, gemm_batch

RELU, DROP, ATOMIC, RELU_BWD, BCAST, SIGMOID, AKM, BKM = 1, 2, 4, 8, 16, 32, 64, 128
WG = AKM | BKM | ATOMIC                       # the weight-gradient form
LAYOUTS = (0, BKM, AKM, WG)
MAXP = 12                                     # GEMM_MAXP
SIGMOID_TOL = 1.98e-7
SEED = 0x1234567_89ABCDEF
f32, f64 = np.float32, np.float64
cdiv = lambda a, b: -(-a // b)


# ---- the launcher's arithmetic, restated -------------------------------------------------------------------------------------------------

def path(M, N, K, flags, lds, aligned, prec, group=()):
    """What launch_gemm_batch and the kernels decide for one problem.  ``lds`` = (lda, ldb, ldc, ldr); ``aligned`` maps A, B, C, bias,
    res to whether the pointer is 16-byte aligned (an absent bias / res is left out); ``group`` = (M, N, K, flags) of the OTHER problems
    of the launch.  -> kernel, pipe, ksplit, kchunk, vec, v4 (None where the epilogue has one form only), blocks, total."""
    lda, ldb, ldc, ldr = lds
    akm, bkm = bool(flags & AKM), bool(flags & BKM)
    every = [(M, N, K, flags)] + list(group)
    al = lambda k: aligned.get(k, True)
    if prec == 0 and all((k if fl & AKM else m) <= 64 for m, n, k, fl in every):
        def blocks(m, n, k, fl):
            tiles = cdiv(m, 16) * cdiv(n, 16)
            return cdiv(tiles, 4) if fl & AKM else tiles
        vec = (akm or (lda % 4 == 0 and al("A"))) and (bkm or (ldb % 4 == 0 and al("B"))) and K % 4 == 0
        return dict(kernel="skinny", pipe=None, ksplit=1, kchunk=K, vec=vec, v4=None, blocks=blocks(M, N, K, flags), total=sum(blocks(*q) for q in every))

    def split(m, n, k, fl):
        ktiles, ksplit = cdiv(k, 32), 1
        if (fl & ATOMIC) and (fl & AKM) and k > 16 * 32:
            ksplit = cdiv(ktiles, 12)
        per = cdiv(ktiles, ksplit)
        return cdiv(ktiles, per), per * 32, cdiv(m, 64) * cdiv(n, 128)
    ksplit, kchunk, tiles = split(M, N, K, flags)
    total = sum(s[0] * s[2] for s in (split(*q) for q in every))
    vec = lda % 4 == 0 and al("A") and (M if akm else K) % 4 == 0 and ldb % 4 == 0 and al("B") and (N if bkm else K) % 4 == 0
    v4 = None
    if not (akm and bkm):
        v4 = (N % 4 == 0 and ldc % 4 == 0 and al("C") and al("bias") and ("res" not in aligned or (ldr % 4 == 0 and al("res")))
              and not flags & (ATOMIC | SIGMOID))
    return dict(kernel="grouped", pipe=4 if total <= 320 else 2, ksplit=ksplit, kchunk=kchunk, vec=vec, v4=v4, blocks=tiles * ksplit, total=total)


# ---- problems and their data -------------------------------------------------------------------------------------------------------------

def P(M, N, K, flags=0, pad=4, off=None, bias=False, res=False, bg=False, aux_scale=1.0, uniform_n=0, lengths=None, site=0, lda=None,
      ldc=None, cname=None, small=False, init=None, no_inv=False):
    """One problem.  ``pad``: ld - extent of A, B, C, res (one number, or a dict with key None for the rest); ``off``: name -> offset of the
    pointer into its array in 4-byte elements; ``res``: the residual, the aux map of RELU_BWD or the per-sample rows of BCAST (samples
    of ``lengths`` rows, or of uniform_n); ``cname``: an output array shared between problems; ``small``: operands in [-1, 1] and bias in
    [-2, 2] (SIGMOID); ``init``: whether C is given integers on entry (default: where it accumulates)."""
    pad = pad if isinstance(pad, dict) else {None: pad}
    return dict(M=M, N=N, K=K, flags=flags, pad=pad, off=off or {}, bias=bias, res=res, bg=bg, aux_scale=aux_scale, uniform_n=uniform_n,
                lengths=lengths, site=site, lda=lda, ldc=ldc, cname=cname, small=small, init=bool(flags & ATOMIC) if init is None else init, no_inv=no_inv)


def lds_of(s):
    akm, bkm, pad = s["flags"] & AKM, s["flags"] & BKM, lambda k: s["pad"].get(k, s["pad"].get(None, 4))
    return (s["lda"] or (s["M"] if akm else s["K"]) + pad("A"), (s["N"] if bkm else s["K"]) + pad("B"), s["ldc"] or s["N"] + pad("C"), s["N"] + pad("res"))


def path_of(specs, i, prec):
    s = specs[i]
    aligned = {k: s["off"].get(k, 0) % 4 == 0 for k in ("A", "B", "C") + (("bias",) if s["bias"] else ()) + (("res",) if s["res"] else ())}
    return path(s["M"], s["N"], s["K"], s["flags"], lds_of(s), aligned, prec, [(q["M"], q["N"], q["K"], q["flags"]) for j, q in enumerate(specs) if j != i])


def at(off, rows, ld, ext):
    """Indices of a rows x ext matrix with leading dimension ld that begins ``off`` elements into its array."""
    return off + np.arange(rows)[:, None] * ld + np.arange(ext)[None, :]


def size(off, rows, ld, ext):
    return max(rows * ld, off + (rows - 1) * ld + ext)


def materialise(specs, seed=0, given=None):
    """-> (probs, ins, outs, init) for raw_calls.gemm / gemm_batch and, per problem, the logical operands.  Every element of every input
    array is drawn, the pad columns too: a read of one shows.  ``given``: name -> the contents of an array instead of drawn ones."""
    probs, ins, outs, init, mats, draw = [], {}, {}, {}, [], lambda name, a: np.asarray((given or {}).get(name, a), f32).reshape(a.shape)
    for i, s in enumerate(specs):
        rs = np.random.RandomState(1000 * seed + 17 * i + s["M"] + s["N"] + s["K"])
        M, N, K, fl, off = s["M"], s["N"], s["K"], s["flags"], lambda k: s["off"].get(k, 0)
        lda, ldb, ldc, ldr = lds_of(s)
        lim = 1 if s["small"] else 3
        (ra, ea), (rb, eb) = ((K, M) if fl & AKM else (M, K)), ((K, N) if fl & BKM else (N, K))
        ins[f"A{i}"] = draw(f"A{i}", rs.randint(-lim, lim + 1, size(off("A"), ra, lda, ea)))
        ins[f"B{i}"] = draw(f"B{i}", rs.randint(-lim, lim + 1, size(off("B"), rb, ldb, eb)))
        Am, Bm = ins[f"A{i}"][at(off("A"), ra, lda, ea)], ins[f"B{i}"][at(off("B"), rb, ldb, eb)]
        m = dict(A=Am.T if fl & AKM else Am, B=Bm if fl & BKM else Bm.T, ldc=ldc, offC=off("C"))
        cn = s["cname"] or f"C{i}"
        q = dict(M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, ldr=ldr, flags=fl, drop_site=s["site"], uniform_n=s["uniform_n"], aux_scale=s["aux_scale"],
                 A=(f"A{i}", off("A")), B=(f"B{i}", off("B")), C=(cn, off("C")))
        nc = size(off("C"), M, ldc, N)
        assert outs.setdefault(cn, ((nc,), f32)) == ((nc,), f32)
        if s["init"] and cn not in init:
            init[cn] = draw(cn, rs.randint(-64, 65, nc))
        if s["bias"]:
            ins[f"bias{i}"] = draw(f"bias{i}", rs.randint(-2 if s["small"] else -64, 3 if s["small"] else 65, off("bias") + N))
            q["bias"], m["bias"] = (f"bias{i}", off("bias")), ins[f"bias{i}"][off("bias"):]
        if s["res"]:
            lengths = s["lengths"] or ([s["uniform_n"]] * cdiv(M, s["uniform_n"]) if s["uniform_n"] else [M])
            rows = len(lengths) if fl & BCAST else M
            lo, hi = (-2, 3) if fl & RELU_BWD else (-64, 65)        # (an aux map with zeros, negatives and positives)
            ins[f"res{i}"] = draw(f"res{i}", rs.randint(lo, hi, size(off("res"), rows, ldr, N)))
            q["res"], m["res"] = (f"res{i}", off("res")), ins[f"res{i}"][at(off("res"), rows, ldr, N)]
            if fl & BCAST:
                m["sample"] = np.repeat(np.arange(rows), lengths)[:M].astype(np.int32)
                assert len(m["sample"]) == M
                if s["lengths"]:
                    ins[f"rs{i}"], q["row_sample"] = m["sample"], (f"rs{i}", 0)
                    if not s["no_inv"]:
                        ins[f"inv{i}"], q["inv_nr"] = (1.0 / np.asarray(lengths, f64)).astype(f32), (f"inv{i}", 0)
                m["inv"] = 1.0 / np.asarray(lengths, f64)
        if s["bg"]:
            outs[f"bg{i}"], init[f"bg{i}"], q["bias_grad"] = ((M,), f32), rs.randint(-64, 65, M).astype(f32), (f"bg{i}", 0)
        probs.append(q)
        mats.append(m)
    return probs, ins, outs, init, mats


def expected(specs, outs, init, mats, fill, drop_p=0.0, seed=0):
    """name -> (what the array holds afterwards as fp32, the same in float64, the bound per element: 0 = bytewise), the problems applied
    in order onto the arrays' contents on entry (``init``, or the fill byte), and the exactness precondition asserted."""
    want = {k: (init[k].copy() if k in init else np.frombuffer(bytes([fill]) * 4 * shape[0], f32).copy()) for k, (shape, _) in outs.items()}
    val = {k: np.zeros(len(w), f64) for k, w in want.items()}
    tol = {k: np.zeros(len(w), f64) for k, w in want.items()}
    mag = {k: (np.abs(init[k]).astype(f64) if k in init else np.zeros(len(w), f64)) for k, w in want.items()}
    for i, (s, m) in enumerate(zip(specs, mats)):
        M, N, fl = s["M"], s["N"], s["flags"]
        A, B = m["A"].astype(np.int64), m["B"].astype(np.int64)
        v, size_, bound = (A @ B).astype(f64), (np.abs(A) @ np.abs(B)).astype(f64), None
        if s["bias"]:
            v, size_ = v + m["bias"][None, :N], size_ + np.abs(m["bias"][None, :N])
        if fl & RELU:
            v = np.maximum(v, 0.0)
        if (fl & DROP) and drop_p > 0:
            idx = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :]
            v, size_ = v * np.where(dropout_keep(seed, s["site"], idx, drop_p), 1.0 / (1.0 - drop_p), 0.0), size_ / (1.0 - drop_p)
        if fl & RELU_BWD:
            v, size_ = v * np.where(m["res"] > 0, f64(s["aux_scale"]), 0.0), size_ * max(1.0, s["aux_scale"])
        elif s["res"] and fl & BCAST:
            r = m["res"][m["sample"]].astype(f64) * m["inv"][m["sample"]][:, None]
            if s["uniform_n"] == 3:
                bound = 2.0 ** -23 * (np.abs(v) + np.abs(r))
            v, size_ = v + r, size_ + np.abs(r)
        elif s["res"]:
            v, size_ = v + m["res"], size_ + np.abs(m["res"])
        if fl & SIGMOID:
            v, bound = 1.0 / (1.0 + np.exp(-v)), np.full(v.shape, SIGMOID_TOL)
        cn, idx = s["cname"] or f"C{i}", at(m["offC"], M, m["ldc"], N)
        mag[cn][idx] += size_
        if fl & ATOMIC:
            v = want[cn][idx].astype(f64) + v
        want[cn][idx], val[cn][idx] = v.astype(f32), v
        tol[cn][idx] = 0.0 if bound is None else bound
        if bound is None:
            assert (want[cn][idx].astype(f64) == v).all()
        if s["bg"]:
            mag[f"bg{i}"] += np.abs(A).sum(1)
            want[f"bg{i}"] = (want[f"bg{i}"].astype(f64) + A.sum(1)).astype(f32)
    assert max(a.max() for a in mag.values()) < 2 ** 24, "the case is not exact by construction"
    return {k: (want[k], val[k], tol[k]) for k in want}


def compare(got, want, what):
    for k, (w32, w64, tol) in want.items():
        g, exact = got[k], tol == 0
        bad = np.flatnonzero(exact & (g.view(np.uint32) != w32.view(np.uint32)))
        assert bad.size == 0, (what, k, "not bytewise the reference at", bad[:8].tolist(), g[bad[:8]].tolist(), w32[bad[:8]].tolist())
        err = np.abs(g.astype(f64) - w64)[~exact]
        assert (err <= tol[~exact]).all(), (what, k, float(err.max()), float((err / tol[~exact]).max()))
    return max([float(np.abs(got[k].astype(f64) - w64)[tol > 0].max()) for k, (w32, w64, tol) in want.items() if (tol > 0).any()] or [0.0])


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
# name -> (problems, what path() says of problem 0 in f32 [and in bf16 where that differs], precisions, the hook, dropout p)
CASES = {}
FORCE = P(65, 1, 1)     # a companion with M > 64: in f32 it puts the whole launch on the tile kernel


def add(name, probs, want, precs=(0, 1), want16=None, batch=False, force=False, drop_p=0.0):
    probs = list(probs) + ([FORCE] if force else [])
    assert name not in CASES and 1 <= len(probs) <= MAXP
    needs_batch = len(probs) > 1 or drop_p > 0 or any(q["aux_scale"] != 1.0 or q["uniform_n"] or q["lengths"] or q["site"] for q in probs)
    CASES[name] = dict(probs=probs, want={0: want, 1: want if want16 is None else want16}, precs=precs, batch=batch or needs_batch, drop_p=drop_p)


def build_cases():
    G, S = dict(kernel="grouped"), dict(kernel="skinny")
    # the skinny / tile switch (f32 only: bf16 always takes the tile kernel)
    for M in (64, 65):
        add(f"switch-M{M}", [P(M, 20, 40, bias=True)], S if M == 64 else G, want16=G)
    for K in (64, 65):
        add(f"switch-K{K}-wg", [P(33, 20, K, WG, bg=True)], S if K == 64 else G, want16=G)
    # the skinny K loop without AKM: 4 waves interleave 16-deep blocks, 8 stages, one trip = 512 k
    for K in (1, 4, 15, 16, 17, 64, 65, 512, 513, 528, 1030, 1536):
        for i, (M, N) in enumerate(((1, 1), (16, 16), (17, 33), (64, 2))):
            add(f"skinny-K{K}-{M}x{N}", [P(M, N, K, BKM if (K + i) % 2 else 0)], dict(kernel="skinny", vec=K % 4 == 0, blocks=cdiv(M, 16) * cdiv(N, 16)), precs=(0,))
    # skinny with AKM: a wave per tile, 4 tiles per block; bias_grad from the first column tile only
    for M, N, blocks in ((48, 16, 1), (40, 24, 2), (8, 100, 2)):
        for K in (5, 64):
            for fl in (WG, AKM | ATOMIC, AKM):
                add(f"skinny-akm-{M}x{N}x{K}-f{fl}", [P(M, N, K, fl, bg=True)], dict(kernel="skinny", blocks=blocks), want16=G)
    for N in (16, 33):
        add(f"skinny-akm-bg-N{N}", [P(20, N, 64, WG, bg=True)], S, want16=G)
    # tile edges of the tile kernel
    for mi, M in enumerate((1, 64, 65, 129)):
        for ni, N in enumerate((1, 4, 127, 128, 129, 130, 257)):
            for ki, K in enumerate((1, 4, 31, 32, 33, 36)):
                fl = LAYOUTS[(mi + ni + ki) % 4]
                add(f"edge-{M}x{N}x{K}-f{fl}", [P(M, N, K, fl, pad=4 if (ni + ki) % 2 else 3, bg=bool(fl & AKM), bias=fl != WG)],
                    dict(kernel="grouped", pipe=4, ksplit=1, blocks=cdiv(M, 64) * cdiv(N, 128)), force=True)
    for K in (32, 64, 96, 128, 160, 161):       # the PIPE = 4 trip count
        for fl in LAYOUTS:
            add(f"trip-K{K}-f{fl}", [P(65, 129, K, fl, bg=bool(fl & AKM))], dict(kernel="grouped", pipe=4, kchunk=32 * cdiv(K, 32)), force=True)
    # tile totals where the XCD remap has q = 0, and r != 0 at 9
    add("tiles-1", [P(64, 128, 72, AKM, bg=True)], dict(kernel="grouped", total=1))
    add("tiles-3", [P(64, 257, 72, AKM, bias=True)], dict(kernel="grouped", total=3))
    add("tiles-9", [P(129, 257, 40, BKM, res=True)], dict(kernel="grouped", total=9))
    # PIPE = 2: more than 320 tiles, the last row tile one row
    for K in (40, 97):
        for fl in (0, BKM):
            add(f"pipe2-K{K}-f{fl}", [P(1281, 2048, K, fl, bias=True)], dict(kernel="grouped", pipe=2, total=336, v4=True, vec=K % 4 == 0))
    # split-K: past 16 K tiles, 12 per block, the last chunk ragged; bias_grad from the first of two column tiles only
    for fl in (WG, AKM | ATOMIC):
        for K, ksplit, kchunk in ((512, 1, 512), (513, 2, 288), (544, 2, 288), (800, 3, 288), (1217, 4, 320), (4001, 11, 384)):
            add(f"splitk-K{K}-f{fl}", [P(65, 129, K, fl, bg=True)], dict(kernel="grouped", ksplit=ksplit, kchunk=kchunk, blocks=4 * ksplit))
    add("splitk-not-without-atomic", [P(65, 129, 800, AKM, bg=True)], dict(kernel="grouped", ksplit=1, kchunk=800))
    # the four layouts x 16-byte loads on and off, each way they switch; non-tight lds throughout
    variants = (("on", {}, {}), ("Kmod4", dict(K=1), {}), ("Mmod4", dict(M=1), {}), ("Nmod4", dict(N=1), {}), ("lda-odd", {}, dict(pad={"A": 3, None: 4})),
                ("ldb-odd", {}, dict(pad={"B": 3, None: 4})), ("A+4B", {}, dict(off={"A": 1})), ("B+4B", {}, dict(off={"B": 1})))
    off_when = {     # variant -> (akm, bkm) -> the loads are scalar
        "grouped": {"on": lambda a, b: False, "Kmod4": lambda a, b: not (a and b), "Mmod4": lambda a, b: a, "Nmod4": lambda a, b: b, "lda-odd": lambda a, b: True,
                    "ldb-odd": lambda a, b: True, "A+4B": lambda a, b: True, "B+4B": lambda a, b: True},
        "skinny": {"on": lambda a, b: False, "Kmod4": lambda a, b: True, "Mmod4": lambda a, b: False, "Nmod4": lambda a, b: False, "lda-odd": lambda a, b: not a,
                   "ldb-odd": lambda a, b: not b, "A+4B": lambda a, b: not a, "B+4B": lambda a, b: not b}}
    for kern, (M, N, K) in (("skinny", (32, 36, 40)), ("grouped", (68, 132, 40))):
        for fl in LAYOUTS:
            for vn, d, kw in variants:
                scalar = off_when[kern][vn](bool(fl & AKM), bool(fl & BKM))
                add(f"vec-{kern}-f{fl}-{vn}", [P(M + d.get("M", 0), N + d.get("N", 0), K + d.get("K", 0), fl, bg=bool(fl & AKM), bias=fl != WG, res=fl == 0, **kw)],
                    dict(kernel=kern, vec=not scalar), precs=(0,) if kern == "skinny" else (0, 1), force=kern == "grouped")
    # epilogues on the 16-byte-store path and on the scalar path, each way the scalar path is reached
    epis = (("relu", dict(flags=RELU)), ("bias-res", dict(bias=True, res=True)), ("relu-bwd", dict(flags=RELU_BWD, res=True, aux_scale=2.0)),
            ("relu-bias-res", dict(flags=RELU, bias=True, res=True)))
    reaches = (("v4", {}), ("N130", dict(N=130)), ("ldc-odd", dict(pad={"C": 3, None: 4})), ("C+4B", dict(off={"C": 1})), ("bias+4B", dict(off={"bias": 1})),
               ("res+4B", dict(off={"res": 1})), ("ldr-odd", dict(pad={"res": 3, None: 4})))
    for en, e in epis:
        for rn, r in reaches:
            if (rn == "bias+4B" and not e.get("bias")) or (rn in ("res+4B", "ldr-odd") and not e.get("res")):
                continue
            for lay in (0, BKM, AKM):
                kw = {k: v for k, v in {**e, **r}.items() if k not in ("flags", "N")}
                add(f"epi-{en}-{rn}-f{lay}", [P(68, r.get("N", 132), 72, lay | e.get("flags", 0), **kw)], dict(kernel="grouped", v4=rn == "v4"))
        kw = {k: v for k, v in e.items() if k != "flags"}
        add(f"epi-{en}-c-orientation", [P(68, 132, 72, AKM | BKM | e.get("flags", 0), **kw)], dict(kernel="grouped", v4=None))       # (no ATOMIC: epilogue_store from the C orientation)
        for lay in (0, BKM):
            add(f"epi-{en}-skinny-f{lay}", [P(33, 36, 40, lay | e.get("flags", 0), **kw)], S, want16=dict(kernel="grouped", v4=True))
    for lay in (BKM | ATOMIC, ATOMIC, AKM | ATOMIC):        # atomic accumulation in the C^T orientation (BKM | ATOMIC: the `nn` form)
        for extra in (0, RELU):
            add(f"epi-atomic-f{lay | extra}", [P(68, 132, 72, lay | extra, bias=True, res=True)], dict(kernel="grouped", v4=False))
            add(f"epi-atomic-skinny-f{lay | extra}", [P(33, 36, 40, lay | extra, bias=True, res=True)], S, want16=dict(kernel="grouped", v4=False))
    for M in (16, 70):      # the head form: one column into column 5 of a 6-wide output, A one quarter of a 4K-wide row
        add(f"head-M{M}", [P(M, 1, 40, bias=True, lda=160, ldc=6, off={"A": 40, "C": 5})], dict(kernel="skinny" if M == 16 else "grouped", v4=None if M == 16 else False),
            want16=dict(kernel="grouped", v4=False))
    # ---- whole groups
    twelve = [P(70, 132, 40, bias=True, res=True), P(16, 20, 33, BKM, pad=3), P(33, 36, 64, WG, bg=True), P(68, 130, 72, AKM, bias=True), P(1, 1, 1),
              P(64, 128, 32, BKM | ATOMIC), P(65, 129, 600, WG, bg=True), P(20, 40, 40, RELU, bias=True), P(48, 16, 8, AKM | ATOMIC, bg=True),
              P(68, 132, 40, RELU_BWD, res=True, aux_scale=2.0), P(30, 36, 36, BCAST, res=True, uniform_n=4),
              P(17, 1, 40, bias=True, lda=160, ldc=6, off={"A": 40, "C": 5})]
    add("group-twelve", twelve, dict(kernel="grouped", pipe=4, v4=True, total=4 + 1 + 1 + 4 + 1 + 1 + 8 + 1 + 1 + 4 + 1 + 1))
    # the tail's shape: AKM problems of 3 and 6 tiles (blocks of (tiles + 3) / 4) between non-AKM ones (blocks of tiles)
    tail = [P(16, 20, 40, bias=True), P(16, 48, 33, WG, bg=True), P(4, 100, 64, BKM), P(32, 48, 64, AKM | ATOMIC, bg=True), P(1, 1, 513), P(64, 2, 16, RELU, bias=True),
            P(8, 100, 5, WG, bg=True), P(17, 33, 65, bias=True, res=True), P(33, 36, 40, BKM | ATOMIC)]
    add("group-tail", tail, dict(kernel="skinny", blocks=2, total=2 + 1 + 7 + 2 + 1 + 4 + 2 + 6 + 9), want16=G)
    add("group-pipe2-splitk", [P(65, 129, 800, WG, bg=True), P(1025, 1280, 8, bias=True), P(1025, 1280, 8, BKM)], dict(kernel="grouped", pipe=2, ksplit=3, total=12 + 170 + 170))
    add("group-shared-accumulator", [P(70, 132, K, BKM | ATOMIC, cname="Cs") for K in (8, 40, 33, 72)], dict(kernel="grouped", v4=False))
    lengths = [1, 2, 4, 8]
    add("group-bcast-small", [P(15, 36, 40, BCAST, res=True, lengths=lengths), P(18, 36, 40, BCAST | RELU, res=True, bias=True, uniform_n=4)], S, want16=dict(kernel="grouped", v4=True))
    add("group-bcast", [P(75, 132, 40, BCAST, res=True, lengths=lengths * 5), P(75, 130, 40, BCAST | BKM, res=True, lengths=lengths * 5), P(15, 36, 40, BCAST, res=True, lengths=lengths),
                        P(70, 132, 40, BCAST, res=True, bias=True, uniform_n=4), P(70, 132, 40, BCAST, res=True, uniform_n=4, off={"res": 1})], dict(kernel="grouped", v4=True))
    add("group-bcast-thirds", [P(17, 36, 40, BCAST, res=True, uniform_n=3), P(20, 33, 40, BCAST | BKM, res=True, uniform_n=3)], S, want16=dict(kernel="grouped", v4=True))
    add("group-bcast-thirds-tiles", [P(70, 132, 40, BCAST, res=True, uniform_n=3), P(70, 130, 40, BCAST, res=True, uniform_n=3)], dict(kernel="grouped", v4=True))
    add("group-dropout-skinny", [P(33, 36, 40, DROP, site=1), P(16, 20, 33, DROP | RELU, bias=True, site=2), P(20, 40, 40, DROP, res=True, site=3)], S,
        want16=dict(kernel="grouped", v4=True), drop_p=0.5)
    add("group-dropout-tiles", [P(68, 132, 40, DROP, site=1), P(68, 130, 40, DROP | RELU, bias=True, site=2), P(70, 132, 72, DROP | BKM, res=True, site=3),
                                P(70, 132, 72, DROP | BKM | ATOMIC, res=True, site=3)], dict(kernel="grouped", v4=True), drop_p=0.5)
    # SIGMOID: pre-activations in [-6, 6]
    for lay in (0, BKM):
        add(f"sigmoid-skinny-f{lay}", [P(33, 36, 4, SIGMOID | lay, bias=True, small=True)], S, want16=dict(kernel="grouped", v4=False))
        add(f"sigmoid-tiles-f{lay}", [P(68, 132, 4, SIGMOID | lay, bias=True, small=True)], dict(kernel="grouped", v4=False))
    for M in (16, 70):
        add(f"sigmoid-head-M{M}", [P(M, 1, 4, SIGMOID, bias=True, small=True, lda=16, ldc=6, off={"A": 4, "C": 5})], dict(kernel="skinny" if M == 16 else "grouped"),
            want16=dict(kernel="grouped", v4=False))


build_cases()

# what the launcher refuses: name -> the problem (C is not given integers: it must come back as its fill)
REFUSED = {
    "wg-bias": P(33, 20, 40, WG, bias=True, init=False), "wg-res": P(33, 20, 40, WG, res=True, init=False), "wg-relu": P(33, 20, 40, WG | RELU, init=False),
    "wg-relu-bwd": P(33, 20, 40, WG | RELU_BWD, res=True, init=False), "wg-dropout": P(33, 20, 40, WG | DROP, init=False),
    "wg-sigmoid": P(33, 20, 40, WG | SIGMOID, init=False), "wg-bcast": P(33, 20, 40, WG | BCAST, res=True, uniform_n=4, init=False),
    "wg-relu-tiles": P(68, 132, 72, WG | RELU, init=False), "wg-bias-splitk": P(65, 129, 800, WG, bias=True, init=False),
    "relu-bwd-no-res": P(33, 20, 40, RELU_BWD), "relu-bwd-no-res-tiles": P(68, 132, 72, RELU_BWD), "bcast-no-res": P(33, 20, 40, BCAST, uniform_n=4),
    "bcast-no-map": P(33, 20, 40, BCAST, res=True), "bcast-no-map-tiles": P(68, 132, 72, BCAST, res=True),
    "bcast-no-inv": P(15, 20, 40, BCAST, res=True, lengths=[1, 2, 4, 8], no_inv=True), "relu-bwd-bcast": P(32, 20, 40, RELU_BWD | BCAST, res=True, uniform_n=4),
}


@functools.lru_cache(maxsize=4)
def prepared(name, fill=0xFF):
    c = CASES[name]
    probs, ins, outs, init, mats = materialise(c["probs"])
    return probs, ins, outs, init, mats, expected(c["probs"], outs, init, mats, fill, c["drop_p"], SEED)


def launch(probs, prec, ins, outs, init, batch, drop_p=0.0, fill=0xFF, rc=None):
    used = {q[k][0] for q in probs for k in ("A", "B", "C", "bias", "res", "bias_grad", "row_sample", "inv_nr") if q.get(k)}
    ins, outs, init = ({k: v for k, v in d.items() if k in used} for d in (ins, outs, init))
    call = gemm_batch(probs, prec, ins, outs, init, drop_p, SEED, rc) if batch else gemm(probs[0], prec, ins, outs, init, rc)
    return execute(call, fill)


# ---- CPU: the predictor, the case list's coverage, the reference ------------------------------------------------------------------------

def test_the_predictor_on_hand_worked_launches():
    t = dict(A=True, B=True, C=True)
    assert path(16, 16, 512, 0, (516, 516, 20, 0), t, 0) == dict(kernel="skinny", pipe=None, ksplit=1, kchunk=512, vec=True, v4=None, blocks=1, total=1)
    assert path(40, 24, 64, WG, (44, 28, 28, 0), t, 0)["blocks"] == 2 and path(40, 24, 65, WG, (44, 28, 28, 0), t, 0)["kernel"] == "grouped"
    assert path(16, 16, 512, 0, (516, 516, 20, 0), t, 1)["kernel"] == "grouped" and path(16, 16, 8, 0, (12, 12, 20, 0), t, 0, [(65, 1, 1, 0)])["kernel"] == "grouped"
    p = path(256, 256, 4000, WG, (256, 256, 256, 0), t, 0)      # tests/test_hip_kernels.py's split-K shape: 125 K tiles, 11 chunks of 12
    assert (p["ksplit"], p["kchunk"], p["blocks"], p["pipe"], p["v4"]) == (11, 384, 4 * 2 * 11, 4, None)
    assert path(256, 256, 512, WG, (256, 256, 256, 0), t, 0)["ksplit"] == 1 and path(256, 256, 513, WG, (256, 256, 256, 0), t, 0)["ksplit"] == 2
    assert path(256, 256, 4000, AKM | BKM, (256, 256, 256, 0), t, 0)["ksplit"] == 1
    assert path(1281, 2048, 40, 0, (44, 44, 2052, 0), t, 1)["pipe"] == 2 and path(1280, 2048, 40, 0, (44, 44, 2052, 0), t, 1)["pipe"] == 4    # 336 and 320 tiles
    assert path(70, 132, 40, 0, (44, 44, 136, 136), dict(t, res=True), 1)["v4"] and not path(70, 132, 40, 0, (44, 44, 136, 135), dict(t, res=True), 1)["v4"]
    assert not path(70, 132, 40, 0, (44, 44, 136, 0), dict(t, bias=False), 1)["v4"] and not path(70, 132, 40, SIGMOID, (44, 44, 136, 0), t, 1)["v4"]
    assert path(72, 132, 40, AKM, (76, 44, 136, 0), t, 1)["vec"] and not path(72, 132, 40, AKM, (76, 44, 136, 0), dict(t, A=False), 1)["vec"]
    assert not path(72, 132, 40, AKM, (74, 44, 136, 0), t, 1)["vec"] and not path(69, 132, 40, AKM, (76, 44, 136, 0), t, 1)["vec"]
    assert path(32, 36, 40, AKM, (35, 44, 40, 0), dict(t, A=False), 0)["vec"] and not path(32, 36, 42, AKM, (36, 44, 40, 0), t, 0)["vec"]      # skinny: k-major reads are scalar anyway


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_takes_the_path_it_was_written_for(name):
    c = CASES[name]
    for prec in c["precs"]:
        got = path_of(c["probs"], 0, prec)
        assert {k: got[k] for k in c["want"][prec]} == c["want"][prec], (name, prec, got)
        assert prec == 0 or got["kernel"] == "grouped"
    assert c["batch"] or len(c["probs"]) == 1


def test_the_cases_have_both_sides_of_every_rule():
    paths = {(n, prec, i): (s, path_of(c["probs"], i, prec)) for n, c in CASES.items() for prec in c["precs"] for i, s in enumerate(c["probs"])}
    have = lambda f: any(f(s, p, prec) for (n, prec, i), (s, p) in paths.items())
    one = lambda n: len(CASES[n]["probs"]) == 1
    # skinny / tile switch at 64 | 65, alone in the launch
    for key, fl in (("M", 0), ("K", AKM)):
        for v, kern in ((64, "skinny"), (65, "grouped")):
            assert any(one(n) and prec == 0 and s[key] == v and (s["flags"] & AKM) == fl and p["kernel"] == kern for (n, prec, i), (s, p) in paths.items()), (key, v)
    for prec in (0, 1):
        assert {p["pipe"] for (n, q, i), (s, p) in paths.items() if q == prec and p["kernel"] == "grouped"} == {2, 4}
        for fl in (WG, AKM | ATOMIC):
            ks = {s["K"]: (p["ksplit"], p["kchunk"] * p["ksplit"] - s["K"]) for (n, q, i), (s, p) in paths.items() if q == prec and s["flags"] == fl and n.startswith("splitk")}
            assert {k: v[0] for k, v in ks.items()} == {512: 1, 513: 2, 544: 2, 800: 3, 1217: 4, 4001: 11}
            assert ks[544][1] == 32 and ks[4001][1] > 192       # ragged last chunks: one tile short, more than half short
        kernels = ("grouped",) if prec else ("skinny", "grouped")
        for kern in kernels:
            for lay in LAYOUTS:
                for vec in (True, False):
                    assert have(lambda s, p, q: q == prec and p["kernel"] == kern and (s["flags"] & (AKM | BKM)) == (lay & (AKM | BKM)) and p["vec"] == vec), (prec, kern, lay, vec)
        for flag in (0, RELU, RELU_BWD, BCAST, DROP):
            for v4 in (True, False):
                assert have(lambda s, p, q: q == prec and p["v4"] is v4 and (flag == 0 or s["flags"] & flag)), (prec, flag, v4)
        for flag in (ATOMIC, SIGMOID):
            assert have(lambda s, p, q: q == prec and p["v4"] is False and s["flags"] & flag)
    for flag in (RELU, RELU_BWD, BCAST, DROP, SIGMOID, ATOMIC):
        assert have(lambda s, p, q: p["kernel"] == "skinny" and s["flags"] & flag and not s["flags"] & AKM), flag
    assert {p["total"] for (n, q, i), (s, p) in paths.items() if p["kernel"] == "grouped"} >= {1, 3, 9, 336}
    # the skinny K loop on both sides of one 16-deep block, of the 4 waves' 64 and of one 512-k trip
    assert {s["K"] for (n, q, i), (s, p) in paths.items() if p["kernel"] == "skinny" and not s["flags"] & AKM} >= {15, 16, 17, 64, 65, 512, 513, 1536}
    assert len(CASES["group-twelve"]["probs"]) == MAXP and {q["flags"] & (AKM | BKM) for q in CASES["group-twelve"]["probs"]} == {0, AKM, BKM, AKM | BKM}
    tail = CASES["group-tail"]["probs"]
    assert len(tail) == 9 and [path_of(tail, i, 0)["blocks"] for i in (1, 3)] == [1, 2] and not tail[0]["flags"] & AKM and not tail[2]["flags"] & AKM
    # non-tight leading dimensions throughout, an offset base for every operand somewhere
    extents = lambda s: (s["M"] if s["flags"] & AKM else s["K"], s["N"] if s["flags"] & BKM else s["K"], s["N"])
    assert all(ld > ext for c in CASES.values() for s in c["probs"][:1] for ld, ext in zip(lds_of(s)[:3], extents(s)))
    assert {k for c in CASES.values() for s in c["probs"] for k, v in s["off"].items() if v % 4} == {"A", "B", "C", "bias", "res"}


def test_the_reference_on_a_hand_worked_problem():
    s = P(2, 3, 2, RELU | ATOMIC, pad=1, bias=True, res=True)
    A, B = np.array([[1, -2], [3, 0]]), np.array([[1, 0, -1], [2, 1, 1]])
    probs, ins, outs, init, mats = materialise([s], given={"A0": [1, -2, 9, 3, 0, 9], "B0": [1, 2, 9, 0, 1, 9, -1, 1, 9], "bias0": [1, -1, 0], "res0": np.arange(8), "C0": [10] * 8})
    assert (mats[0]["A"] == A).all() and (mats[0]["B"] == B).all() and probs[0]["lda"] == 3 and probs[0]["ldc"] == 4
    want = expected([s], outs, init, mats, 0xFF)["C0"][0]
    hand = np.maximum(A @ B + [1, -1, 0], 0) + np.arange(8).reshape(2, 4)[:, :3] + 10
    assert (want.reshape(2, 4)[:, :3] == hand).all() and (want.reshape(2, 4)[:, 3] == 10).all() and hand[0, 0] == 10 and hand[1, 0] == 18
    akm = P(2, 3, 2, WG, pad=1, bg=True)
    probs, ins, outs, init, mats = materialise([akm])
    want = expected([akm], outs, init, mats, 0xFF)
    assert (want["bg0"][0] == init["bg0"] + mats[0]["A"].sum(1)).all() and (mats[0]["A"] == ins["A0"].reshape(2, 3)[:, :2].T).all()
    d = P(4, 4, 1, DROP, site=3)
    probs, ins, outs, init, mats = materialise([d])
    want = expected([d], outs, init, mats, 0xFF, 0.5, SEED)["C0"][0][at(0, 4, 8, 4)]
    keep = dropout_keep(SEED, 3, np.arange(16), 0.5).reshape(4, 4)
    assert 0 < keep.sum() < 16 and (want == np.where(keep, 2.0, 0.0) * (mats[0]["A"] @ mats[0]["B"])).all()
    assert np.isnan(expected([d], outs, init, mats, 0xFF, 0.5, SEED)["C0"][0].reshape(4, 8)[:, 4:]).all()       # untouched pad columns hold the fill


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_is_exact_by_construction(name):
    prepared(name)      # (asserts the 2**24 precondition and that every exact value is an fp32 number)


# ---- on the device ----------------------------------------------------------------------------------------------------------------------

def launches_by_kind(run):
    """(what ``run`` returns, launches of the tile kernel, launches of the skinny kernel) by the library's own launch timing: kind 0 and
    kind 5 of camo_prof_kind.  The two kernels compute the same exact result, so the outputs cannot tell which one ran."""
    from camouflage_multimodal_amd import _lib
    L, n = _lib.lib(), [ctypes.c_int32(-1), ctypes.c_int32(-1)]
    _lib.check(L.camo_prof_begin(8), "camo_prof_begin")
    try:
        got = run()
    finally:
        _lib.check(L.camo_prof_end(None, None, None), "camo_prof_end")
    for kind, k in zip((0, 5), n):
        _lib.check(L.camo_prof_kind(kind, None, ctypes.byref(k), None), "camo_prof_kind")
    return got, n[0].value, n[1].value


def run_case(name, prec):
    c = CASES[name]
    probs, ins, outs, init, mats, want = prepared(name)
    got, tiles, skinny = launches_by_kind(lambda: launch(probs, prec, ins, outs, init, c["batch"], c["drop_p"]))
    assert (tiles, skinny) == ((0, 1) if path_of(c["probs"], 0, prec)["kernel"] == "skinny" else (1, 0)), (name, prec, tiles, skinny)
    return compare(got, want, (name, prec))


@pytest.mark.gpu
@pytest.mark.parametrize("name,prec", [(n, p) for n, c in CASES.items() if not n.startswith(("sigmoid", "group-twelve")) for p in c["precs"]])
def test_gemm_is_the_exact_reference(name, prec):
    run_case(name, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", (0, 1))
def test_twelve_mixed_problems_in_one_launch_are_what_each_gives_alone(prec):
    probs, ins, outs, init, mats, want = prepared("group-twelve")
    got = launch(probs, prec, ins, outs, init, True)
    compare(got, want, ("group-twelve", prec))
    for i, q in enumerate(probs):
        alone = launch([q], prec, ins, outs, init, True)
        for k, a in alone.items():
            assert a.tobytes() == got[k].tobytes(), (i, k)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", (0, 1))
def test_sigmoid_against_float64(prec):
    """Bound SIGMOID_TOL = 1.98e-7: 4 x the worst error measured on an MI355X over these cases (4.944e-8), far below the 2.4e-3 by which a
    unit error of the pre-activation moves the result."""
    worst = max(run_case(n, prec) for n in CASES if n.startswith("sigmoid"))
    assert worst > 0
    print(f"sigmoid: worst error {worst:.3e} (bound {SIGMOID_TOL:.1e})")
    assert SIGMOID_TOL <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("prec", (0, 1))
@pytest.mark.parametrize("K", (512, 513))
@pytest.mark.parametrize("flags", (WG, AKM | ATOMIC))
def test_the_split_k_threshold_is_seen_through_one_rounding(flags, K, prec):
    """A split and an unsplit launch give the same bytes on exact data, so this one case leaves the exact range on purpose: C holds 2**24
    on entry and every product sum is 1 (from k = 0) + 1 (from k = K - 1).  One block adds 2 and C is 2**24 + 2; two K chunks add 1 each,
    and 2**24 + 1 rounds back to 2**24 (ties to even) both times, in either order.  K = 512 must not split and K = 513 must."""
    M, N = 65, 129
    ksplit, kchunk = (path(M, N, K, flags, (M + 4, N + 4, N + 4, 0), {}, prec)[k] for k in ("ksplit", "kchunk"))
    assert (ksplit, kchunk) == ((1, 512) if K == 512 else (2, 288)) and (K - 1) // kchunk == ksplit - 1
    A, B = np.zeros((K, M + 4), f32), np.ones((K, N + 4) if flags & BKM else (N, K + 4), f32)
    A[0, :M] = A[K - 1, :M] = 1
    prob = dict(M=M, N=N, K=K, lda=M + 4, ldb=B.shape[1], ldc=N + 4, flags=flags, A=("A", 0), B=("B", 0), C=("C", 0))
    c0 = np.full(M * (N + 4), 2.0 ** 24, f32)
    got = execute(gemm(prob, prec, {"A": A.reshape(-1), "B": B.reshape(-1)}, {"C": ((M * (N + 4),), f32)}, {"C": c0}), 0xFF)["C"].reshape(M, N + 4)
    assert (got[:, N:] == 2.0 ** 24).all() and (got[:, :N] == (2.0 ** 24 + 2 if ksplit == 1 else 2.0 ** 24)).all(), (np.unique(got[:, :N]).tolist(), ksplit)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_launches_return_an_error_and_touch_nothing(name):
    from camouflage_multimodal_amd import _lib
    s = REFUSED[name]
    simple = not (s["uniform_n"] or s["lengths"])
    for prec in (0, 1):
        for specs, batch in (([s], True), ([P(16, 20, 8), s], True)) + ((([s], False),) if simple else ()):
            probs, ins, outs, init, mats = materialise(specs)
            rc = []
            got = launch(probs, prec, ins, outs, init, batch, fill=0xA5, rc=rc)
            assert rc[0] != 0 and len(_lib.lib().camo_last_error()) > 0, (name, prec, rc)
            for k, a in got.items():
                assert k in init or a.tobytes() == bytes([0xA5]) * a.nbytes, (name, k)
                assert k not in init or a.tobytes() == init[k].tobytes(), (name, k)


@pytest.mark.gpu
def test_a_group_of_thirteen_is_refused_and_bad_arguments_are_named():
    from camouflage_multimodal_amd import _lib
    specs = [P(16, 20, 8)] * 13
    probs, ins, outs, init, mats = materialise(specs)
    rc = []
    got = launch(probs, 0, ins, outs, init, True, fill=0xA5, rc=rc)
    assert rc[0] == -1 and b"gemm batch" in _lib.lib().camo_last_error() and all(a.tobytes() == bytes([0xA5]) * a.nbytes for a in got.values())
    for bad in (dict(M=0), dict(K=0), dict(A=None), dict(C=None)):
        rc = []
        got = launch([dict(probs[0], **bad)], 0, ins, outs, init, True, fill=0xA5, rc=rc)
        assert rc[0] == -1 and all(a.tobytes() == bytes([0xA5]) * a.nbytes for a in got.values()), bad
    want = expected(specs[:12], {k: v for k, v in outs.items() if k != "C12"}, init, mats[:12], 0xFF)
    compare(launch(probs[:12], 0, ins, outs, init, True), want, "twelve are accepted")


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(70, 130, 37), (200, 256, 128)])
def test_bf16_operands_are_rounded_to_nearest_even(M, N, K):
    """Real operands at prec = 1 against the float64 product of the oracle's RNE-bf16-rounded operands, at tests/test_hip_gemm16.py's
    bound 2e-6 (|a| @ |b| + 1).  Truncation instead of RNE would sit near 2**-9 |a| @ |b|, a thousand times the bound."""
    worst = 0.0
    for fl in LAYOUTS:
        rs = np.random.RandomState(M + K + fl)
        Am, Bm = rs.standard_normal((M, K)).astype(f32), rs.standard_normal((K, N)).astype(f32)
        lda, ldb, ldc = (M if fl & AKM else K) + 4, (N if fl & BKM else K) + 4, N + 4
        A, B = np.zeros((K if fl & AKM else M, lda), f32), np.zeros((K if fl & BKM else N, ldb), f32)
        A[:, :lda - 4], B[:, :ldb - 4] = (Am.T if fl & AKM else Am), (Bm if fl & BKM else Bm.T)
        c0 = np.zeros(M * ldc, f32)
        prob = dict(M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, flags=fl, A=("A", 0), B=("B", 0), C=("C", 0))
        got = execute(gemm(prob, 1, {"A": A.reshape(-1), "B": B.reshape(-1)}, {"C": ((M * ldc,), f32)}, {"C": c0} if fl & ATOMIC else None), 0xFF)["C"].reshape(M, ldc)
        a, b = bf16_round(Am).astype(f64), bf16_round(Bm).astype(f64)
        ratio = np.abs(got[:, :N] - a @ b) / (2e-6 * (np.abs(a) @ np.abs(b) + 1))
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1, (fl, float(ratio.max()))
        assert (got[:, N:] == 0).all() if fl & ATOMIC else np.isnan(got[:, N:]).all()
    print(f"bf16 rounding {M}x{N}x{K}: worst error / bound {worst:.3f}")
