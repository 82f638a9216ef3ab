"""The march launched alone at the flagship shape (4096 rays, 1536 nodes, P = 12, 512^3 table): dense and sparse alternating, HIP events."""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from samplenerfro_amd import ops, _lib, synthetic as syn
dev = torch.device("cuda:0")
B, N, P, G = 4096, 1536, 12, 512
o, d = syn.sphere_rays(B)
o = torch.from_numpy(o).to(dev); d = torch.from_numpy(d).to(dev)
jit = torch.from_numpy(np.arange(0, N, P, dtype=np.int32) + np.random.default_rng(1).integers(0, P, N // P).astype(np.int32)).to(dev)
for scene in ("uniform", "refractive sphere"):
    spec = _lib.Grid.make([G] * 3, [-1.5] * 3, [1.5] * 3, "reference")
    if scene == "uniform":
        grid = torch.ones((G, G, G), device=dev)
    else:
        grid = ops.grid_prefilter(torch.from_numpy(syn.scale_ior(syn.sphere_grid(G, 1.5, 0.6), 0.5).astype(np.float32)).to(dev), 9, 3.0)
    table = ops.grid_build_table(grid, spec)
    del grid
    pd = torch.empty((N, B, 4), device=dev); dr = torch.empty_like(pd)
    pd2 = torch.zeros((N, B, 4), device=dev); dr2 = torch.zeros_like(pd2)
    ops.march(table, spec, o, d, 2.0, 6.0, N, out=(pd, dr))
    ops.march_sparse(table, spec, o, d, 2.0, 6.0, N, jit, P, out=(pd2, dr2))
    torch.cuda.synchronize()
    at = jit.long()
    print(f"{scene}: sparse == dense at the sampled nodes: {bool(torch.equal(pd[at], pd2[at]) and torch.equal(dr[at], dr2[at]))}")
    res = {"dense": [], "sparse": []}
    for rnd in range(5):
        for kind in ("dense", "sparse"):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(21)]
            ev[0].record()
            for i in range(20):
                if kind == "dense":
                    ops.march(table, spec, o, d, 2.0, 6.0, N, out=(pd, dr))
                else:
                    ops.march_sparse(table, spec, o, d, 2.0, 6.0, N, jit, P, out=(pd2, dr2))
                ev[i + 1].record()
            torch.cuda.synchronize()
            res[kind].append(float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(20)])))
    for kind in ("dense", "sparse"):
        print(f"{scene} G={G}: {kind:6s} ms per launch, median of 20, five rounds: " + " ".join("%.4f" % x for x in res[kind]) + "  | median %.4f" % np.median(res[kind]))
    del table, pd, dr, pd2, dr2
