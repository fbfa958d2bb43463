"""What is_sat costs, timed on the device's host at the config-2 shape (a 2048-byte message) and at one 64-byte message: SpartanSNARK.is_sat as a whole
(z, the three products, the residual pass, the recomputed commitment), Shape.is_sat on the same shape and assignment (products + residual pass, no
commitment), the residual kernel alone by the HIP events attached to its dispatch (with the bytes it moves over that time), sp_multiply_vec alone on the
same shape and z - the floor: the check cannot do without the products - and prove + verify on the same state, which is the only way to learn the
same fact without is_sat. Medians of `runs` calls after `warmup`. Writes a Markdown table (profiles/is_sat.md is this output).
usage: python tools/sat_timing.py [--out profiles/is_sat.md] [--runs 20] [--warmup 3]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spartan2_amd import frontend, hip, host  # noqa: E402


def med(f, runs, warmup):
    for _ in range(warmup):
        f()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def residual_kernel(ctx, f, runs):
    """(mean device ms, algorithmic bytes) of one r1cs_residual launch over `runs` calls of f, by the events attached to the dispatch"""
    ctx.stats_filter("r1cs_residual")
    ctx.reset_stats(True)
    for _ in range(runs):
        f()
    ctx.synchronize()
    ms, n, nbytes = ctx.kernel_stats("r1cs_residual")
    ctx.reset_stats(False)
    ctx.stats_filter("")
    return ms / max(n, 1), nbytes / max(n, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "is_sat.md"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    ctx = hip.Context(0)
    rng = np.random.default_rng(2)
    lines = [f"# is_sat on the MI355X: medians of {a.runs} calls after {a.warmup} warm-up calls, ms", "",
             "`is_sat` = SpartanSNARK.is_sat (z + products + residual pass + PCS::commit of the committed rows); `Shape.is_sat` = products + residual pass;",
             "`residual kernel` = k_r1cs_residual alone by HIP events, with its algorithmic bytes (96 B a row + the bitmap) over that time;",
             "`multiply_vec` = sp_multiply_vec alone on the same shape and z (the floor); `prove + verify` = the same fact without is_sat.", "",
             "| message | constraints | variables | is_sat | Shape.is_sat | residual kernel | residual bytes | residual GB/s | multiply_vec | prove | verify | prove + verify |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in (2048, 64):
        msg = rng.bytes(n)
        inst = frontend.sha256_circuit(msg)
        tape = np.random.default_rng(1).integers(0, 256, size=(8192, 64), dtype=np.uint8)
        sn = host.SpartanSNARK(ctx, inst)
        used = sn.prep_prove(tape)
        rep = sn.is_sat()
        assert rep.ok, rep
        d = sn.dims
        N, M = d["num_cons"], d["num_shared"] + d["num_precommitted"] + d["num_rest"]
        # the same shape and assignment through the ABI's own classes
        mats, dims = host.pad_shape(inst)
        shape = hip.Shape(ctx, mats, dims)
        z = np.concatenate([host.padded_witness_limbs(dims, inst.witness), host.mont_limbs_from_u64(np.concatenate([[1], inst.publics]).astype(np.uint64))])
        zt = hip.Table.from_host(ctx, z)
        outs = [hip.Table.zeros(ctx, N) for _ in range(3)]
        assert shape.is_sat(zt).ok

        def mv():
            shape.multiply_vec(zt, *outs)
            ctx.synchronize()

        words = {}

        def prove():
            words["w"] = sn.prove(tape[used:])[0]

        def verify():
            assert sn.verify(words["w"]) == 0

        def both():
            prove()
            verify()

        t_sat = med(lambda: sn.is_sat(), a.runs, a.warmup)
        t_shape = med(lambda: shape.is_sat(zt), a.runs, a.warmup)
        k_ms, k_bytes = residual_kernel(ctx, lambda: shape.is_sat(zt), a.runs)
        t_mv = med(mv, a.runs, a.warmup)
        t_prove = med(prove, a.runs, a.warmup)
        t_verify = med(verify, a.runs, a.warmup)
        t_both = med(both, a.runs, a.warmup)
        lines.append(f"| {n} B | {N} | {M} | {t_sat:.3f} | {t_shape:.3f} | {k_ms:.4f} | {int(k_bytes)} | {k_bytes / (k_ms * 1e-3) / 1e9 if k_ms > 0 else 0:.0f} | {t_mv:.3f} | "
                     f"{t_prove:.3f} | {t_verify:.3f} | {t_both:.3f} |")
        print(lines[-1], flush=True)
        sn.close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
