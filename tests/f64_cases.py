"""Deterministic inputs shared by the CPU self-checks of oracle/f64_refs.py (tests/test_f64_refs.py) and the GPU tests that hold the
loss and optimizer kernels to it (tests/test_hip_loss.py, tests/test_hip_optimizer.py): what the CPU tests show the bounds catch
is caught on exactly the inputs the kernels are run on."""
import numpy as np

LOSS_CLASSES = (1, 2, 3, 8, 9, 64)
LOSS_BATCHES = (1, 63, 64, 65, 1000)
MAGNITUDES = (0.0, 0.1, 2.0, 6.0, 12.0, 20.0, 40.0, 87.0, 100.0)
EDGE_LOGITS = (0.0, 1e-4, -1e-4, 5.0, -5.0, 17.0, -17.0, 40.0, -40.0, 100.0, -100.0)
EDGE_LABELS = (0.0, 1.0, 0.3)
SCORES = (0.0, 1e-7, 0.5, 1.0 - 1e-7, 1.0)
SCORE_LABELS = (0.0, 1.0, 0.3, 0.5, None)          # None: the label equal to the score


def _place(row, yy, where, mag, C):
    """Make class yy the largest / the smallest / tied for the maximum with class (yy + 1) % C."""
    if C == 1:
        return row
    others = np.delete(row, yy)
    step = 0.5 * mag if mag > 0 else 0.0
    if where == 0:
        row[yy] = others.max() + step
    elif where == 1:
        row[yy] = others.min() - step
    else:
        row[yy] = row[(yy + 1) % C] = row.max() + 0.25 * mag
    return row


def loss_grid(C):
    """-> outs [N, 2C+2] float32, y int64 [N], e float32 [N], s float32 [N], init_scale bool [N] (rows whose logits are within a
    few tenths of zero, the scale every other test of the loss runs at).  Rows: every label x every magnitude x the true class
    largest / smallest / tied (mask and instance logits placed differently); all logits equal at +-magnitude; one row with a logit
    gap of 120 (pt underflows in float32, the cross entropy must stay finite).  The edge logit x label and the score x label
    combinations cycle with periods 33 and 25 over the rows."""
    rs = np.random.RandomState(1234 + C)
    rows = []                                       # (mask logits, instance logits, y, init_scale)
    for yy in range(C):
        for mag in MAGNITUDES:
            for where in range(3):
                a = _place(rs.uniform(-1, 1, C) * mag, yy, where, mag, C)
                b = _place(rs.uniform(-1, 1, C) * mag, yy, (where + 1) % 3, mag, C)
                rows.append((a, b, yy, mag <= 0.1))
    for mag in MAGNITUDES:
        for sign in (1.0, -1.0):
            rows.append((np.full(C, sign * mag), np.full(C, -sign * mag), (len(rows) * 7) % C, mag <= 0.1))
    if C > 1:
        a = np.zeros(C); a[0] = -60.0; a[1] = 60.0
        rows.append((a, a[::-1].copy(), 0, False))
    N = len(rows)
    assert N >= 33
    outs = np.zeros((N, 2 * C + 2), np.float32)
    y = np.zeros(N, np.int64); e = np.zeros(N, np.float32); s = np.zeros(N, np.float32); init = np.zeros(N, bool)
    for i, (a, b, yy, ini) in enumerate(rows):
        outs[i, :C] = a; outs[i, C:2 * C] = b; y[i] = yy
        ec = i % 33
        outs[i, 2 * C] = EDGE_LOGITS[ec % 11]; e[i] = EDGE_LABELS[ec // 11]
        sc = i % 25
        outs[i, 2 * C + 1] = np.float32(SCORES[sc % 5])
        lab = SCORE_LABELS[sc // 5]
        s[i] = outs[i, 2 * C + 1] if lab is None else lab
        init[i] = ini and abs(EDGE_LOGITS[ec % 11]) < 1.0
    return outs, y, e, s, init


def loss_calls(C):
    """The calls of one class count: (B, row indices into loss_grid(C)).  B = 1000 walks the whole grid (wrapping round); the
    small batches start at different rows."""
    N = len(loss_grid(C)[1])
    calls = []
    for B in LOSS_BATCHES:
        if B == 1000:
            for start in range(0, N, 1000):
                calls.append((B, (start + np.arange(B)) % N))
        else:
            calls.append((B, (37 * B + np.arange(B)) % N))
    return calls


# ------------------------------------------------------------------------------------------------------------------ clip + AdamW
HYPERS = {
    "default": dict(lr=5e-4, wd=1e-4, b1=0.9, b2=0.999, eps=1e-8, max_norm=1.0),
    "lr1e-2_wd0.1": dict(lr=1e-2, wd=0.1, b1=0.9, b2=0.999, eps=1e-8, max_norm=1.0),
    "wd0": dict(lr=5e-4, wd=0.0, b1=0.9, b2=0.999, eps=1e-8, max_norm=1.0),
    "eps1e-3": dict(lr=5e-4, wd=1e-4, b1=0.9, b2=0.999, eps=1e-3, max_norm=1.0),
    "betas.5_.9": dict(lr=5e-4, wd=1e-4, b1=0.5, b2=0.9, eps=1e-8, max_norm=1.0),
}
STEPS = (1, 2, 10, 1000, 100000)
GRAD_KINDS = ("below", "near", "above", "zero", "span")
SIZES = (1, 3, 4, 5, 1023, 262147, 2 * 1048576 + 5)


def adamw_grad(n, kind, seed, max_norm=1.0):
    """float32 gradient of n elements: global norm 1e-2 x max_norm (``below``: no clipping), within 1e-3 of it (``near``: 1.0002 x),
    1e3 x (``above``); all zero; ``span``: magnitudes log-uniform from 2e-12 to 0.1 and one element of 1e3 -- the norm is ~1e3, the
    clip coefficient ~1e-3, so every clipped element stays >= 1e-15 and its square a normal float32."""
    rs = np.random.RandomState(500 + seed)
    if kind == "zero":
        return np.zeros(n, np.float32)
    if kind == "span":
        mag = 10.0 ** rs.uniform(np.log10(2e-12), -1.0, n)
        g = mag * np.where(rs.uniform(size=n) < 0.5, -1.0, 1.0)
        g[(3 * n) // 4] = 1e3
        if n >= 3:
            g[0] = 2e-12; g[n // 2] = -0.1
        return g.astype(np.float32)
    g = rs.standard_normal(n)
    g[np.abs(g) < 1e-3] = 1e-3                     # (no element so small that its clipped square leaves the normal range)
    target = dict(below=1e-2, near=1.0002, above=1e3)[kind] * max_norm
    return (g * (target / np.sqrt((g * g).sum()))).astype(np.float32)


def adamw_state(n, seed):
    """p ~ U(+-1); m, v of a plausible late state: m ~ 1e-3 N(0, 1), v = m^2 x U(.5, 2) + 1e-12, every tenth element untouched so
    far (m = v = 0)."""
    rs = np.random.RandomState(900 + seed)
    p = rs.uniform(-1, 1, n)
    m = 1e-3 * rs.standard_normal(n)
    v = m * m * rs.uniform(0.5, 2.0, n) + 1e-12
    fresh = rs.uniform(size=n) < 0.1
    m[fresh] = 0.0; v[fresh] = 0.0
    return p.astype(np.float32), m.astype(np.float32), v.astype(np.float32)


def adamw_cross_cases():
    """Every hyper-parameter set x step x gradient kind x zero_grads at n = 1023 (the scalar tail: 1023 % 4 = 3)."""
    for hname in HYPERS:
        for step in STEPS:
            for gi, kind in enumerate(GRAD_KINDS):
                for zg in (0, 1):
                    yield hname, step, kind, zg, 11 * step % 97 + gi
