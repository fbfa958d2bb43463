"""What verify_batch saves, timed on the device's host at the config-2 shape (sha256_circuit(bytes(2048)): 2^20 constraints). One key, one proof per
message through prep_prove_sha256 (so the proofs differ); then for K in 1, 4, 16, 64, in ONE process and alternating the two forms repetition by
repetition: K sequential SpartanSNARK.verify calls against one verify_batch call over the same K proofs. Host clock around calls that end synchronised
(both forms return verdicts the host has read); median and min .. max of `runs` repetitions after `warmup`.
k_matrix_evals_batched alone: by the HIP events attached to its dispatch in this process, and - with --kernel-stats - from the kernel_stats CSV of a
separate run under `rocprofv3 --kernel-trace --stats -- python tools/verify_batch_timing.py --trace-run 16` (a tracer distorts host timings, so the two
never share a run). Its algorithmic bytes (the structure once per chunk, one 32-byte gather per entry and proof, T_x once per matrix and proof) are
computed here from sp_shape_info. Writes a Markdown note (profiles/verify_batch.md is this output plus the compiler's resource line).
usage: python tools/verify_batch_timing.py [--out profiles/verify_batch.md] [--runs 20] [--warmup 3] [--kernel-stats kernel_stats.csv] [--msg-len 2048]"""
import argparse
import csv
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spartan2_amd import frontend, hip, host  # noqa: E402

KS = (1, 4, 16, 64)
KERNEL = "k_matrix_evals_batched"


def chunk_bytes(nnz, nrows, kc):
    """algorithmic bytes of one launch over kc proofs: indices + codes and the row pointers of both classes once, then per proof a 32-byte gather per
    entry and the T_x element of every row of every matrix"""
    return 5 * nnz + 24 * nrows + kc * (32 * nnz + 96 * nrows)


def batch_bytes(nnz, nrows, k, kc):
    full, rest = divmod(k, kc)
    return full * chunk_bytes(nnz, nrows, kc) + (chunk_bytes(nnz, nrows, rest) if rest else 0)


def make_proofs(sn, n, msg_len):
    rng = np.random.default_rng(7)
    tape = np.random.default_rng(1).integers(0, 256, size=(8192, 64), dtype=np.uint8)
    proofs = []
    for _ in range(n):
        used = sn.prep_prove_sha256(rng.bytes(msg_len), tape)
        proofs.append(sn.prove(tape[used:])[0])
    return proofs


def kernel_row(path):
    """(calls, average us) of the kernel in a rocprofv3 kernel_stats CSV"""
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if KERNEL in row.get("Name", ""):
                return int(row["Calls"]), float(row["AverageNs"]) / 1e3
    raise SystemExit(f"{KERNEL} is not in {path}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batch.md"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--msg-len", type=int, default=2048)
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats CSV of a separate rocprofv3 --kernel-trace --stats run of --trace-run")
    ap.add_argument("--trace-run", type=int, default=0, metavar="K", help="only run a few verify_batch calls over K proofs (the program to put under rocprofv3)")
    a = ap.parse_args()
    ctx = hip.Context(0)
    sn = host.SpartanSNARK(ctx, frontend.sha256_circuit(bytes(a.msg_len)))
    kc = hip.matrix_evals_chunk()
    if a.trace_run:
        proofs = make_proofs(sn, a.trace_run, a.msg_len)
        for _ in range(5):
            assert sn.verify_batch(proofs) == [0] * len(proofs)
        sn.close()
        ctx.close()
        return
    proofs = make_proofs(sn, max(KS), a.msg_len)
    d = sn.dims
    N, nnz = d["num_cons"], sum(sn.shape_info["nnz"])
    lines = [f"# verify_batch on the MI355X, {a.msg_len}-byte messages: {N} constraints, {nnz} entries in A, B, C", "",
             f"One process, the two forms alternating; median (min .. max) of {a.runs} repetitions after {a.warmup}, host clock, ms. `sequential` = K calls of",
             "SpartanSNARK.verify (unchanged by verify_batch: the figure of the commit before it); `batch` = one SpartanSNARK.verify_batch call.",
             f"KC = {kc} proofs per launch of {KERNEL}.", "",
             "| K | sequential, total | batch, total | sequential, per proof | batch, per proof | batch / sequential | chunks | fallback |", "|---|---|---|---|---|---|---|---|"]
    for K in KS:
        b = proofs[:K]

        def seq():
            for p in b:
                assert sn.verify(p) == 0

        def bat():
            codes, _, info = sn.verify_batch(b, info=True)
            assert codes == [0] * K and info["opening_batched_ok"] == 1, (codes, info)
            return info

        for _ in range(a.warmup):
            seq()
            info = bat()
        ts, tb = [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            seq()
            t1 = time.perf_counter()
            bat()
            t2 = time.perf_counter()
            ts.append((t1 - t0) * 1e3)
            tb.append((t2 - t1) * 1e3)
        ms, mb = statistics.median(ts), statistics.median(tb)
        lines.append(f"| {K} | {ms:.3f} ({min(ts):.3f} .. {max(ts):.3f}) | {mb:.3f} ({min(tb):.3f} .. {max(tb):.3f}) | {ms / K:.3f} | {mb / K:.3f} | {mb / ms:.2f} | "
                     f"{info['matrix_chunks']} | {info['fallback_proofs']} |")
        print(lines[-1], flush=True)
    # the kernel alone: events attached to its dispatches, full chunks (K = 16)
    ctx.stats_filter("matrix_evals_batched")
    ctx.reset_stats(True)
    for _ in range(a.runs):
        sn.verify_batch(proofs[:16])
    ctx.synchronize()
    k_ms, k_n, k_bytes = ctx.kernel_stats("matrix_evals_batched")
    ctx.reset_stats(False)
    ctx.stats_filter("")
    per = k_ms / max(k_n, 1)
    want = chunk_bytes(nnz, N, kc)
    assert k_n == 0 or k_bytes // k_n == want, (k_bytes // max(k_n, 1), want)
    lines += ["", f"`{KERNEL}`, one launch over {kc} proofs: {want} algorithmic bytes ({want / 2**20:.1f} MiB; the single-proof route moves "
              f"{kc * (36 * nnz + 96 * N + 3 * 64 * N) / 2**20:.1f} MiB for the same {kc} proofs: structure per proof, three product tables written and read back with T_x).",
              f"- HIP events on the dispatch, {k_n} launches in this process: {per * 1e3:.1f} us a launch, {want / (per * 1e-3) / 1e9 if per > 0 else 0:.0f} GB/s algorithmic"]
    if a.kernel_stats:
        calls, avg_us = kernel_row(a.kernel_stats)
        lines.append(f"- rocprofv3 --kernel-trace --stats, separate run ({calls} launches): {avg_us:.1f} us a launch, {want / (avg_us * 1e-6) / 1e9:.0f} GB/s algorithmic")
    sn.close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
