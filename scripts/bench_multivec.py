#!/usr/bin/env python3
"""Standalone benchmark of exact multivector (late-interaction / MaxSim) search (mi355_multivec_search,
k_multivec_scan); not part of bench.py.

Default shape (ColBERT-like): 1 M rows of 16-64 vectors (16 + Binomial(48, 1/3): mean 32) x 128-d, query sets of 32
vectors, k 10, batches of 1, 16 and 64 query sets, the column as f32 and as bf16.  The column is generated on the device
and the handle scans it in place (borrowed device column).  Prints ONE JSON line with, per (dtype, batch): query sets per
second, the device time of a call (scan kernel + query prep + selection + merge, HIP events on the handle's stream: an
upper bound of the scan kernel's time), the achieved fraction of the f32 matrix peak (2 * n_qvec * n_vectors * dim FLOP
per query set against 157.3 TF) and the column bytes / call time; and a numpy CPU baseline (float32 matmul + segment
minima on a sample of rows, at most 16 threads) extrapolated to the whole column.

    python scripts/bench_multivec.py [--rows N] [--dim D] [--n-qvec Q] [--k K] [--batches 1,16,64]
                                     [--dtypes f32,bf16] [--steps S] [--warmup W] [--cpu-rows R]
"""
import argparse
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):  # the CPU baseline: at most 16 threads
    os.environ[_v] = str(min(16, int(os.environ.get(_v, "16") or 16)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_MATRIX_PEAK = 157.3e12  # v_mfma_f32_32x32x2_f32 peak, FLOP/s


def cpu_baseline(np, col, off, q, rows):
    """Query sets per second of a numpy float32 MaxSim over the first `rows` rows, extrapolated to the column."""
    n_rows = len(off) - 1
    rows = min(rows, n_rows)
    x = col[: int(off[rows])]
    xn = np.sqrt((x * x).sum(1))
    starts = off[:rows].astype(np.int64)
    t0 = time.perf_counter()
    for qs in q:
        qn = np.sqrt((qs * qs).sum(1))
        s = 1.0 - (qs @ x.T) / (qn[:, None] * xn[None, :])
        m = np.minimum.reduceat(s, starts, axis=1)
        d = m.sum(0)
        np.argpartition(d, 10)[:10]
    t = (time.perf_counter() - t0) / len(q)
    return {"query_sets_per_s": 1.0 / (t * n_rows / rows), "sample_rows": rows, "sample_query_sets": len(q),
            "threads": int(os.environ["OMP_NUM_THREADS"]), "note": "numpy f32 matmul + reduceat on a sample, extrapolated"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--n-qvec", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-rows", type=int, default=20_000)
    a = ap.parse_args()

    import numpy as np
    import torch

    import lancedb_amd
    from lancedb_amd import _abi

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    n, dim, nq_v, k = a.rows, a.dim, a.n_qvec, a.k
    lens = 16 + rng.binomial(48, 1.0 / 3.0, size=n)
    off = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    n_vec = int(off[-1])
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    col = torch.randn((n_vec, dim), generator=g, device=dev, dtype=torch.float32)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    batches = [int(b) for b in a.batches.split(",")]
    qpool = torch.randn((2, max(batches), nq_v, dim), generator=g, device=dev, dtype=torch.float32)
    stream = torch.cuda.Stream(device=dev)  # (not the null stream: its handle value 0 means "the handle's own stream")
    res = {"metric": f"query sets/sec, exact multivector {n} rows x {n_vec / n:.1f} vectors x {dim}, n_qvec {nq_v}, k {k}",
           "config": {"n_rows": n, "n_vectors": n_vec, "dim": dim, "n_qvec": nq_v, "k": k, "batches": batches,
                      "lengths": "16 + Binomial(48, 1/3)", "data": "N(0, 1) elements"},
           "model": {"flop_per_query_set": 2.0 * nq_v * n_vec * dim, "peak_flops": F32_MATRIX_PEAK,
                     "ceiling_query_sets_per_s": F32_MATRIX_PEAK / (2.0 * nq_v * n_vec * dim)},
           "runs": []}
    for dname in a.dtypes.split(","):
        dtype = {"f32": _abi.DTYPE_F32, "bf16": _abi.DTYPE_BF16}[dname]
        c = col if dtype == _abi.DTYPE_F32 else col.to(torch.bfloat16)
        torch.cuda.synchronize()
        t_open = time.perf_counter()
        mv = lancedb_amd.MultiVectorFlat(c, d_off, dtype=dtype)
        t_open = time.perf_counter() - t_open
        mv.set_stream(stream.cuda_stream)
        params = _abi.make_params(k=k)
        col_bytes = n_vec * dim * (4 if dtype == _abi.DTYPE_F32 else 2)
        for B in batches:
            out = (torch.empty((B, k), dtype=torch.int64, device=dev), torch.empty((B, k), dtype=torch.float32, device=dev),
                   torch.empty((B,), dtype=torch.int32, device=dev))
            for i in range(max(a.warmup, 1)):
                mv.search(qpool[i % 2, :B], params, out=out)
            torch.cuda.synchronize()
            mv.sync()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * a.steps)]
            t0 = time.perf_counter()
            for i in range(a.steps):
                ev[2 * i].record(stream)
                mv.search(qpool[i % 2, :B], params, out=out)
                ev[2 * i + 1].record(stream)
            stream.synchronize()
            wall = (time.perf_counter() - t0) / a.steps
            call_ms = sorted(ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(a.steps))[a.steps // 2]
            flop = 2.0 * nq_v * n_vec * dim * B
            res["runs"].append({
                "dtype": dname, "batch": B, "open_s": t_open,
                "query_sets_per_s": B / wall, "ms_per_call": wall * 1e3, "device_ms_per_call": call_ms,
                "f32_matrix_peak_frac": flop / (call_ms * 1e-3) / F32_MATRIX_PEAK,
                "column_bytes_per_s": col_bytes / (call_ms * 1e-3),
            })
        mv.close()
        del c
    cs = col[: int(off[min(a.cpu_rows, n)])].cpu().numpy()
    res["cpu_numpy_baseline"] = cpu_baseline(np, cs, off, qpool[0, :2].cpu().numpy(), a.cpu_rows)
    best = max(res["runs"], key=lambda r: r["query_sets_per_s"])
    res.update({"value": best["query_sets_per_s"], "unit": "query sets/s", "best_run": {"dtype": best["dtype"], "batch": best["batch"]}})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
