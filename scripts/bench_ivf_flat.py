#!/usr/bin/env python3
"""Standalone benchmark of IVF_FLAT search (MI355_INDEX_IVF_FLAT, k_ivf_flat_scan); not part of bench.py.

Default shape (the issue's model): 10 M x 768 f32 rows, nlist 1220 (rows / 8192), nprobes 20, k 10, batches of 2048
queries.  The column is generated on the device (rows = centroid + noise, partitions of equal length) and the
IVF_FLAT handle scans it in place (borrowed device column).  Prints ONE JSON line: QPS, the per-stage device times of
a step, the achieved fraction of the VALU roofline of the exact scan (one sub + one fma per element at the f32 vector
peak of 157 TF: ~39 T elements/s) and the QPS of the flat bf16-GEMM path over the same column.

    python scripts/bench_ivf_flat.py [--rows N] [--dim D] [--nlist L] [--nprobe P] [--k K] [--batch B]
                                     [--steps S] [--warmup W] [--no-flat]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_ELEMS_PER_S = 157e12 / 4  # f32 vector peak / (sub + fma = 2 ops = 4 flops per element)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=0, help="0 = rows / 8192")
    ap.add_argument("--nprobe", type=int, default=20)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-flat", action="store_true", help="skip the flat-GEMM comparison")
    a = ap.parse_args()

    import numpy as np
    import torch

    import lancedb_amd
    from lancedb_amd import _abi

    dev = torch.device("cuda", 0)
    n, dim, B, k = a.rows, a.dim, a.batch, a.k
    nlist = a.nlist or max(1, n // 8192)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    cen = torch.randn((nlist, dim), generator=g, device=dev, dtype=torch.float32)
    lens = np.full(nlist, n // nlist, np.int64)
    lens[: n - lens.sum()] += 1
    po = np.zeros(nlist + 1, np.uint64)
    po[1:] = np.cumsum(lens)
    col = torch.empty((n, dim), device=dev, dtype=torch.float32)
    part = torch.repeat_interleave(torch.arange(nlist, device=dev), torch.from_numpy(lens).to(dev))
    step = 1_000_000
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        col[r0:r1] = cen[part[r0:r1]] + 0.5 * torch.randn((r1 - r0, dim), generator=g, device=dev, dtype=torch.float32)
    del part
    P = 2
    qpool = [(cen[torch.randint(0, nlist, (B,), generator=g, device=dev)] +
              0.5 * torch.randn((B, dim), generator=g, device=dev, dtype=torch.float32)).contiguous() for _ in range(P)]
    torch.cuda.synchronize()

    t_open = time.perf_counter()
    ix = lancedb_amd.IvfFlatIndex(cen, po, col, None, metric="l2")
    t_open = time.perf_counter() - t_open
    stream = torch.cuda.current_stream().cuda_stream
    ix.set_stream(stream)
    params = _abi.make_params(k=k, nprobe_min=a.nprobe, nprobe_max=a.nprobe)
    out = (torch.empty((B, k), dtype=torch.int64, device=dev), torch.empty((B, k), dtype=torch.float32, device=dev),
           torch.empty((B,), dtype=torch.int32, device=dev))
    for i in range(max(a.warmup, 1)):
        ix.search(qpool[i % P], params, out=out)
    torch.cuda.synchronize()
    # untimed-by-events run for the QPS, then one profiled pass for the stage split
    t0 = time.perf_counter()
    for i in range(a.steps):
        ix.search(qpool[i % P], params, out=out)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    qps = B * a.steps / elapsed
    ix.configure(profile=2)
    for i in range(a.steps):
        ix.search(qpool[i % P], params, out=out)
    st = ix.stats()
    launches = max(st["scan_launches"], 1)
    stage = {name: st["us_" + name] / launches for name in ("coarse", "select", "plan", "scan", "merge", "total")}
    assert st["scan_variant"] == _abi.SCAN_IVF_FLAT, "the IVF_FLAT scan did not run"
    rows_per_step = st["vectors_scanned"] / launches
    elems_per_step = rows_per_step * dim
    scan_s = stage["scan"] * 1e-6
    res = {
        "metric": f"queries/sec, IVF_FLAT {n}x{dim} f32, nlist {nlist}, nprobes {a.nprobe}, k {k}, batch {B}",
        "value": qps, "unit": "queries/s", "steps": a.steps, "ms_per_step": elapsed / a.steps * 1e3,
        "open_s": t_open,
        "config": {"n_rows": n, "dim": dim, "nlist": nlist, "nprobe": a.nprobe, "k": k, "batch_queries": B, "dtype": "f32",
                   "metric": "l2", "data": "synthetic: equal partitions, rows = centroid + N(0, 0.25)"},
        "stage_us_per_step": stage,
        "rows_scanned_per_query": rows_per_step / B,
        "roofline": {
            "bound": "valu", "model": "one sub + one fma per (query, row, element) at 157 TF f32 vector peak",
            "peak_elements_per_s": VALU_ELEMS_PER_S,
            "ceiling_qps": VALU_ELEMS_PER_S / (elems_per_step / B),
            "scan_elements_per_s": elems_per_step / max(scan_s, 1e-12),
            "scan_frac": elems_per_step / max(scan_s, 1e-12) / VALU_ELEMS_PER_S,
            "step_frac": qps / (VALU_ELEMS_PER_S / (elems_per_step / B)),
        },
    }
    ix.close()
    del ix
    if not a.no_flat:
        fl = lancedb_amd.FlatIndex(col, dtype=_abi.DTYPE_F32, device=0)
        fl.set_stream(stream)
        fparams = _abi.make_params(k=k, nprobe_min=1, nprobe_max=1, metric=_abi.METRIC_L2)
        fl.configure(path="filter")
        for i in range(max(a.warmup, 1)):
            fl.search(qpool[i % P], fparams, out=out)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.steps):
            fl.search(qpool[i % P], fparams, out=out)
        torch.cuda.synchronize()
        fe = time.perf_counter() - t0
        res["flat_gemm_same_column"] = {"value": B * a.steps / fe, "unit": "queries/s", "ms_per_step": fe / a.steps * 1e3,
                                        "path": fl.info()[0], "note": "bf16 MFMA filter (bf16 shadow of the f32 column) + exact re-rank"}
        fl.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
