"""The device-event timer of the dev_*_bench.py tools: a window is ``iters`` calls between two device events, a figure the smallest
of ``windows`` windows, with the largest beside it.  Microseconds per call throughout.  torch is imported when a timer runs, so the
tools' ``host`` modes need no GPU."""


def window(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters): fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def timed(fn, iters, windows=5, warm=20):
    """(smallest, largest) microseconds per call of ``windows`` windows, after ``warm`` calls."""
    import torch
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    us = [window(fn, iters) for _ in range(windows)]
    return min(us), max(us)


def alternate(fns, iters, windows=5):
    """{name: (smallest, largest) microseconds per call}: every function warmed up, then one window each in turn, ``windows`` times."""
    import torch
    for fn in fns.values():
        for _ in range(20): fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            us[k].append(window(fn, iters))
    return {k: (min(v), max(v)) for k, v in us.items()}
