"""What prep_prove_batch buys, timed on the device's host at the config-2 shape (2048-byte messages, one key): K prep states as (a) K sequential
prep_prove_sha256 calls (`prep_prove_batch(one_pass=False)`, the loop), (b) one one-pass batch call with BOTH batched phases (sp_hyrax_commit_batch and,
with chunked_matvec, sp_multiply_vec_chunked), (c) (b) with per_state_commit (one sp_hyrax_commit per state), (d) (b) with per_state_matvec (one
sp_multiply_vec per state) - (d) is what the driver takes by default, chosen by this measurement. One process, the legs alternating; median
(min .. max) of `runs` repetitions after `warmup`, host clock; the states of the previous repetition are freed outside the timed region. Then the
batch's phases, the kernels by HIP events (the new ones beside k_msm_binary_rows and k_spmv3<true> of one state), and the end-to-end figure: messages
in, proofs out, as prep_prove_batch + prove_batch against sequential prep_prove_sha256 + prove. Writes a Markdown report (profiles/prep_prove_batch.md
holds this output).
usage: python tools/prep_batch_timing.py [--out FILE] [--runs 20] [--warmup 3] [--ks 1,4,16] [--no-kernels] [--no-end-to-end]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spartan2_amd import frontend, hip, host  # noqa: E402

MSG_LEN = 2048
PHASE_NAMES = ("witness", "commit", "tables", "matvec", "scratch", "total")
LEGS = [("a", dict(one_pass=False)), ("b", dict(chunked_matvec=True)), ("c", dict(chunked_matvec=True, per_state_commit=True)), ("d", dict(per_state_matvec=True))]


def stat(ts):
    return statistics.median(ts), min(ts), max(ts)


def fmt(s):
    return f"{s[0]:.3f} ({s[1]:.3f} .. {s[2]:.3f})"


def stalls(ts):
    """repetitions that took more than ten times the median: an allocation call that stalled, not the work measured"""
    m = statistics.median(ts)
    return sum(1 for t in ts if t > 10 * m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prep_prove_batch.md"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ks", default="1,4,16")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-end-to-end", action="store_true")
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    kmax = max(ks)
    ctx = hip.Context(0)
    rng = np.random.default_rng(2)
    sn = host.SpartanSNARK(ctx, frontend.sha256_circuit(bytes(MSG_LEN)))
    msgs = [rng.bytes(MSG_LEN) for _ in range(kmax)]
    prep_tapes = [np.random.default_rng(100 + k).integers(0, 256, size=(1024, 64), dtype=np.uint8) for k in range(kmax)]
    prove_tapes = [np.random.default_rng(200 + k).integers(0, 256, size=(8192, 64), dtype=np.uint8) for k in range(kmax)]
    d = sn.dims

    def prep(K, **kw):
        sn._free_batch()
        ctx.synchronize()
        t0 = time.perf_counter()
        sn.prep_prove_batch(prep_tapes[:K], msgs=msgs[:K], **kw)
        dt = (time.perf_counter() - t0) * 1e3
        return dt, (dict(sn.batch_prep_phases) if kw.get("one_pass", True) else None)

    lines = [f"# prep_prove_batch on the MI355X, {MSG_LEN}-byte messages: {d['num_cons']} constraints", "",
             f"command: python tools/prep_batch_timing.py --runs {a.runs} --warmup {a.warmup} --ks {a.ks}" + (" --no-kernels" if a.no_kernels else "")
             + (" --no-end-to-end" if a.no_end_to_end else ""), "",
             f"One process, the legs alternating; median (min .. max) of {a.runs} repetitions after {a.warmup}, host clock, ms. (a) = K sequential",
             "`prep_prove_sha256` calls (the loop: `one_pass=False`); (b) = one one-pass `prep_prove_batch` call with both batched phases",
             "(`chunked_matvec=True`); (c) = (b) with `per_state_commit=True`: one `sp_hyrax_commit` per state instead of `sp_hyrax_commit_batch`; (d) = (b) with",
             "`per_state_matvec=True`: one `sp_multiply_vec` per state instead of `sp_multiply_vec_chunked` - what the driver takes by default. The states of the",
             "repetition before are freed outside the timed region."]
    names = [n for n, _ in LEGS]
    cols = [f"({n}) total" for n in names] + [f"({n}) per state" for n in names] + ["(b) / (a)", "(b) / (c)", "(b) / (d)", "(d) / (a)", "reps over 10 x median, (a) / (b) / (c) / (d)"]
    lines += ["", "| K | " + " | ".join(cols) + " |", "|---|" + "---|" * len(cols)]
    phase_lines = []
    for K in ks:
        ts = {n: [] for n in names}
        ph = {n: [] for n in names}
        for rep in range(a.warmup + a.runs):
            for n, kw in LEGS:
                dt, phases = prep(K, **kw)
                if rep >= a.warmup:
                    ts[n].append(dt)
                    if phases:
                        ph[n].append(phases)
        s = {n: stat(v) for n, v in ts.items()}
        cells = [fmt(s[n]) for n in names] + [f"{s[n][0] / K:.3f}" for n in names]
        cells += [f"{s['b'][0] / s[o][0]:.2f}" for o in ("a", "c", "d")] + [f"{s['d'][0] / s['a'][0]:.2f}", " / ".join(str(stalls(ts[n])) for n in names)]
        lines.append(f"| {K} | " + " | ".join(cells) + " |")
        print(lines[-1], flush=True)
        for n in ("b", "c", "d"):
            phase_lines.append(f"| {K} | ({n}) | " + " | ".join(fmt(stat([p[k] for p in ph[n]])) for k in PHASE_NAMES) + " |")
    lines += ["", "Phases of the one-pass calls above, ms for the whole batch (host clock between the phases; device work still queued when a phase ends is",
              "waited for in `scratch`, which ends with the one synchronise), median (min .. max) over the same repetitions:", "",
              "| K | leg | " + " | ".join(PHASE_NAMES) + " |", "|---|---|" + "---|" * len(PHASE_NAMES)] + phase_lines
    sn._free_batch()

    if not a.no_kernels:  # the launches of one state and of one batch, by the HIP events around them
        classes = ("commit_canon_classify", "msm_binary_rows", "fixed_base", "spmv", "spmv_multi", "sha256_witness")
        for title, K, kw in ((f"one state (`prep_prove_sha256`)", 1, dict(one_pass=False)), (f"one batch, K = {kmax}, both phases batched", kmax, dict(chunked_matvec=True)),
                             (f"K = {kmax} with `per_state_commit` and `per_state_matvec`", kmax, dict(per_state_commit=True, per_state_matvec=True))):
            prep(K, **kw)
            sn._free_batch()
            ctx.synchronize()
            ctx.reset_stats(True)
            prep(K, **kw)
            ctx.synchronize()
            lines += ["", f"The launches of {title} (HIP events around each launch):", "", "| kernel class | launches | device ms | ms per state |", "|---|---|---|---|"]
            for what in classes:
                ms, launches, _ = ctx.kernel_stats(what)
                if launches:
                    lines.append(f"| {what} | {launches} | {ms:.4f} | {ms / K:.4f} |")
            ctx.reset_stats(False)
            sn._free_batch()

    if not a.no_end_to_end:  # messages in, proofs out
        held = []  # the sequential leg's states: freed outside the timed region, as the batch's are

        def sequential(K):
            for k in range(K):
                sn.prep_prove_sha256(msgs[k], prep_tapes[k])
                sn.prove(prove_tapes[k])
                held.append(sn.ps)
                sn.ps = None

        def batched(K):
            sn.prep_prove_batch(prep_tapes[:K], msgs=msgs[:K])
            sn.prove_batch(prove_tapes[:K])

        lines += ["", "## Messages in, proofs out", "",
                  "(e) = K times `prep_prove_sha256` + `prove`, one after the other; (f) = `prep_prove_batch` (the driver's default) + `prove_batch`. Same process,",
                  "alternating, the same repetitions; ms; the states of both legs are freed outside the timed region. Every state is proven once, so with the",
                  "default `SPARTAN_PREP_TABLES=lazy` every prove queues the build of its state's FixedBaseMul tables behind itself (a few ms of device work that the NEXT call waits behind); the second table is the same with",
                  "`SPARTAN_PREP_TABLES=off`."]
        for mode in ("lazy", "off"):
            os.environ["SPARTAN_PREP_TABLES"] = mode
            lines += ["", f"`SPARTAN_PREP_TABLES={mode}`:", "", "| K | (e) total | (f) total | (e) per proof | (f) per proof | (f) / (e) | reps over 10 x median, (e) / (f) |", "|---|---|---|---|---|---|---|"]
            for K in ks:
                ts = {"e": [], "f": []}
                for rep in range(a.warmup + a.runs):
                    for n, f in (("e", sequential), ("f", batched)):
                        sn._free_batch()
                        while held:
                            host.lib().ss_prep_free(held.pop())
                        ctx.synchronize()
                        t0 = time.perf_counter()
                        f(K)
                        dt = (time.perf_counter() - t0) * 1e3
                        if rep >= a.warmup:
                            ts[n].append(dt)
                e, f = stat(ts["e"]), stat(ts["f"])
                lines.append(f"| {K} | {fmt(e)} | {fmt(f)} | {e[0] / K:.3f} | {f[0] / K:.3f} | {f[0] / e[0]:.2f} | {stalls(ts['e'])} / {stalls(ts['f'])} |")
                print(lines[-1], flush=True)
        os.environ.pop("SPARTAN_PREP_TABLES", None)
        while held:
            host.lib().ss_prep_free(held.pop())
    sn.close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
