"""Developer aid / measurement of the Region-Graph GNN's loss and gradients with frozen batch norm: one
loss_and_gradients call against extract_node_embeddings + node_heads on the same graphs, in the same run, at 16 and at 128 graphs of
~410 nodes.  --bn adds the batch-statistics call (running statistics updated) beside the frozen one, in the same run.
--dropout P adds the call with dropout P in all three classes beside the p = 0 call of each mode, in the same run.
  python tools/dev/dev_rg_train_bench.py [--bn] [--dropout P] [graphs_per_batch ...]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from camouflage_multimodal_amd import RegionGraphData, RegionGraphGNN
from oracle import rg_gnn_oracle as RO


def timed(fn, it=30, warm=5):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(it): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / it


ARGS = sys.argv[1:]
BN = "--bn" in ARGS
DROP = float(ARGS[ARGS.index("--dropout") + 1]) if "--dropout" in ARGS else 0.0
if "--dropout" in ARGS:
    del ARGS[ARGS.index("--dropout"):ARGS.index("--dropout") + 2]
m = RegionGraphGNN().cuda().eval()
for G in [int(a) for a in ARGS if a != "--bn"] or [16, 128]:
    gs = [RO.make_graph(int(n), seed=i) for i, n in enumerate(np.random.RandomState(0).randint(303, 518, size=G))]
    off = np.cumsum([0] + [g[0].shape[0] for g in gs])
    x = torch.from_numpy(np.concatenate([g[0] for g in gs])).cuda()
    ei = torch.from_numpy(np.concatenate([g[1] + off[i] for i, g in enumerate(gs)], axis=1)).cuda()
    ew = torch.from_numpy(np.concatenate([g[2] for g in gs])).cuda()
    data = RegionGraphData(x, ei, ew[:, None])
    N = x.shape[0]
    rs = np.random.RandomState(1)
    mt, it_ = (torch.from_numpy(rs.randint(0, 2, size=N).astype(np.int32)).cuda() for _ in range(2))
    et = torch.from_numpy(rs.uniform(0, 1, size=N).astype(np.float32)).cuda()
    fwd = timed(lambda: m.node_heads(m.extract_node_embeddings(data)))
    trn = timed(lambda: m.loss_and_gradients(data, mt, it_, et))
    print(f"{G} graphs / {N} nodes / {ei.shape[1] + N} CSR entries: forward (embeddings + heads) {fwd * 1e6:.1f} us, "
          f"loss_and_gradients {trn * 1e6:.1f} us = {trn / fwd:.2f} x the forward (both include their CSR builds)")
    if BN:
        bn = timed(lambda: m.loss_and_gradients(data, mt, it_, et, batch_stats=True))
        print(f"    with batch statistics {bn * 1e6:.1f} us = {bn / trn:.2f} x the frozen call, + {(bn - trn) * 1e6:.1f} us")
    if DROP > 0:
        # p = 0 and p = DROP interleaved, twice: what the second round repeats is the difference, what it does not is drift
        for name, kw in (("frozen", {}),) + ((("batch statistics", dict(batch_stats=True)),) if BN else ()):
            for rnd in (1, 2):
                base = timed(lambda: m.loss_and_gradients(data, mt, it_, et, **kw))
                drp = timed(lambda: m.loss_and_gradients(data, mt, it_, et, dropout=DROP, seed=rnd, **kw))
                print(f"    {name}, round {rnd}: p = 0 {base * 1e6:.1f} us, dropout {DROP:g} {drp * 1e6:.1f} us = {drp / base:.3f} x, "
                      f"+ {(drp - base) * 1e6:.1f} us")
