"""What prove_batch buys, timed on the device's host at the config-2 shape (2048-byte messages, one key): K proofs as (a) K sequential `prove` calls
(the headline driver), (b) K sequential reference-order proves (one thread, the reference's statement order: what prove_batch restates), (c) one
`prove_batch` call, (d) one `prove_batch(per_proof_opening=True)` call: (c) with the openings as K sp_hyrax_prove calls, what prove_batch did before
sp_hyrax_prove_batch, (e) / (f) / (g) one `prove_batch` call with evals_rx + poly_ABC and the rest commitments both forced to their batched forms except
(e) per_proof_polyabc=True, (f) per_proof_rest_commit=True, (g) neither: the three legs the driver's two defaults are decided by (the batched form is
taken from the smallest K at which (g)'s median lies below the minimum of (e), respectively (f)), (h) / (i) one `prove_batch` call with the openings begun
ahead of the sum-checks (opening_ahead=True: sp_hyrax_prove_batch_begin / _rows / _finish) and the same batch with opening_ahead=False (the ahead form
becomes the default from the smallest K at which (h)'s median lies below (i)'s minimum). One process, the legs alternating; median (min .. max) of `runs` repetitions after `warmup`, host clock; the phases of (c) and
(d) per K, the batched opening's kernels and the launches of one sp_poly_abc_batch beside the same K as sp_eq_table_into + sp_poly_abc pairs, by HIP
events. Then the lockstep cubic
kernels alone at 2^20-element tables, 16 instances, by the HIP events attached to their dispatches (sp_ctx_kernel_stats), beside the single-proof
k_bind_eval_cubic_stream of the same run. Writes a Markdown report (profiles/prove_batch.md holds this output for this commit and its parent).
--no-batch: legs (a) and (b) only - they need nothing of prove_batch, so this form also runs on the commit before it (the baseline column).
usage: python tools/prove_batch_timing.py [--out FILE] [--runs 20] [--warmup 3] [--ks 1,4,16] [--no-batch] [--no-options] [--no-ahead] [--no-kernels]"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spartan2_amd import frontend, hip, host  # noqa: E402

MSG_LEN = 2048


def stat(ts):
    return statistics.median(ts), min(ts), max(ts)


def fmt(s):
    return f"{s[0]:.3f} ({s[1]:.3f} .. {s[2]:.3f})"


def kernels_alone(ctx, lines, count=16, ell=20):
    """the lockstep cubic kernels at `count` instances of 2^ell elements, and the single-proof prover on one instance, by HIP events"""
    n = 1 << ell
    rng = np.random.default_rng(5)
    data = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)  # (canonical: the top limb stays below the modulus')
    tabs = [[hip.Table.from_host(ctx, data) for _ in range(3)] for _ in range(count)]
    taus = rng.integers(0, 1 << 62, size=(count, ell, 4), dtype=np.uint64)
    claims = rng.integers(0, 1 << 62, size=(count, 4), dtype=np.uint64)

    def lockstep():
        for t3 in tabs:
            for t in t3:
                t.set_len(n)  # (bound down to one element by the run before: the contents no longer matter, the traffic is the same)
        trs = [hip.Transcript(ctx, b"t") for _ in range(count)]
        hip.sumcheck_cubic3_lockstep(ctx, claims, taus, [t[0] for t in tabs], [t[1] for t in tabs], [t[2] for t in tabs], trs)

    def single():
        for t in tabs[0]:
            t.set_len(n)
        hip.sumcheck_cubic3(ctx, claims[0], taus[0], *tabs[0], hip.Transcript(ctx, b"t"))

    lockstep()
    single()
    ctx.reset_stats(True)
    t0 = time.perf_counter()
    lockstep()
    t_lock = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    single()
    t_single = (time.perf_counter() - t0) * 1e3
    ctx.synchronize()
    lines += ["", f"## The lockstep cubic kernels alone: {count} instances of 2^{ell} elements (HIP events on the dispatches, one sum-check each)", "",
              f"host clock: lockstep sum-check of {count} instances {t_lock:.3f} ms ({t_lock / count:.3f} ms an instance); single-proof sp_sumcheck_cubic3 of one instance "
              f"{t_single:.3f} ms", "", "| kernel class | launches | device ms | algorithmic bytes | GB/s algorithmic |", "|---|---|---|---|---|"]
    for what in ("ls_eval_cubic", "ls_bind_eval_cubic", "ls_sum_partials", "eval_cubic", "bind_stream_cubic", "bind"):
        ms, launches, nbytes = ctx.kernel_stats(what)
        if launches:
            lines.append(f"| {what} | {launches} | {ms:.4f} | {nbytes} | {nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0:.0f} |")
    ctx.reset_stats(False)
    for t3 in tabs:
        for t in t3:
            t.free()


def poly_abc_launches(ctx, sn, lines, K, reps=5):
    """the launches of one sp_poly_abc_batch over K proofs, and the same K as back-to-back sp_eq_table_into + sp_poly_abc, by the HIP events on the dispatches"""
    mats, dims = host.pad_shape(frontend.sha256_circuit(bytes(MSG_LEN)))
    shape = hip.Shape(ctx, mats, dims)
    N, M = dims["num_cons"], dims["num_shared"] + dims["num_precommitted"] + dims["num_rest"]
    ell = N.bit_length() - 1
    rng = np.random.default_rng(9)
    r_x = rng.integers(0, 1 << 62, size=(K, ell, 4), dtype=np.uint64)
    r = rng.integers(0, 1 << 62, size=(K, 4), dtype=np.uint64)
    outs = [hip.Table.zeros(ctx, 2 * M) for _ in range(K)]
    rx = hip.Table.zeros(ctx, N)

    def batched():
        shape.poly_abc_batch(r_x, r, 2 * M, outs)

    def per_proof():
        for k in range(K):
            hip.check(hip.lib().sp_eq_table_into(ctx.h, hip.p64(np.ascontiguousarray(r_x[k])), ctypes.c_size_t(ell), rx.h))
            shape.poly_abc(rx, r[k], 2 * M, outs[k])

    lines += ["", f"The launches of one `sp_poly_abc_batch` over K = {K} proofs (chunks of {hip.poly_abc_batch_chunk()}), and the same K as back-to-back `sp_eq_table_into` + `sp_poly_abc`",
              f"(HIP events on the dispatches, sums over {reps} calls after one warm-up; the per-proof path's pyramid launch, two blocks, carries no events):", "",
              "| path | kernel class | launches | device ms | device ms a proof | algorithmic bytes | GB/s algorithmic |", "|---|---|---|---|---|---|---|"]
    for path, f, classes in (("batched", batched, ("eq_levels_batch", "eq_table_batch", "poly_abc_batch")), ("per proof", per_proof, ("eq_table", "poly_abc"))):
        f()
        ctx.synchronize()
        ctx.reset_stats(True)
        for _ in range(reps):
            f()
        ctx.synchronize()
        total = 0.0
        for what in classes:
            ms, launches, nbytes = ctx.kernel_stats(what)
            total += ms
            lines.append(f"| {path} | {what} | {launches} | {ms:.4f} | {ms / (reps * K):.4f} | {nbytes} | {nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0:.0f} |")
        lines.append(f"| {path} | all | | {total:.4f} | {total / (reps * K):.4f} | | |")
        ctx.reset_stats(False)
    for t in outs + [rx]:
        t.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prove_batch.md"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ks", default="1,4,16")
    ap.add_argument("--no-batch", action="store_true", help="legs (a) and (b) only: runs on the commit before prove_batch too")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-options", action="store_true", help="without legs (e), (f), (g): runs on the commit before sp_poly_abc_batch too")
    ap.add_argument("--no-ahead", action="store_true", help="without legs (h), (i): runs on the commit before sp_hyrax_prove_batch_begin too")
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    kmax = max(ks)
    ctx = hip.Context(0)
    rng = np.random.default_rng(2)
    sn = host.SpartanSNARK(ctx, frontend.sha256_circuit(bytes(MSG_LEN)))
    # kmax prepared states of the one key, through the entry point every commit has: the state is taken out of the object after each prep_prove
    states = []
    for k in range(kmax):
        sn.prep_prove_sha256(rng.bytes(MSG_LEN), np.random.default_rng(100 + k).integers(0, 256, size=(1024, 64), dtype=np.uint8))
        states.append((sn.ps, sn.publics))
        sn.ps = None
    tapes = [np.random.default_rng(200 + k).integers(0, 256, size=(8192, 64), dtype=np.uint8) for k in range(kmax)]
    d = sn.dims

    def sequential(K, reference_order):
        for k in range(K):
            sn.ps, sn.publics = states[k]
            sn.set_flags(reference_order=reference_order)
            sn.prove(tapes[k])
        sn.ps = None

    def batch(K, per_proof_opening=False, **kw):
        for k in range(K):  # (a batch of one is handed to prove: the headline driver)
            sn.ps = states[k][0]
            sn.set_flags(reference_order=False)
        sn.ps = None
        if per_proof_opening:
            kw["per_proof_opening"] = True
        return sn.prove_batch(tapes[:K], states=states[:K], **kw)[1]

    legs = [("a", lambda K: sequential(K, False)), ("b", lambda K: sequential(K, True))]
    if not a.no_batch:
        legs += [("c", batch), ("d", lambda K: batch(K, True))]
    if not a.no_batch and not a.no_options:
        legs += [("e", lambda K: batch(K, per_proof_polyabc=True, per_proof_rest_commit=False)), ("f", lambda K: batch(K, per_proof_polyabc=False, per_proof_rest_commit=True)),
                 ("g", lambda K: batch(K, per_proof_polyabc=False, per_proof_rest_commit=False))]
    if not a.no_batch and not a.no_ahead:
        legs += [("h", lambda K: batch(K, opening_ahead=True)), ("i", lambda K: batch(K, opening_ahead=False))]
    lines = [f"# prove_batch on the MI355X, {MSG_LEN}-byte messages: {d['num_cons']} constraints", "",
             f"command: python tools/prove_batch_timing.py --runs {a.runs} --warmup {a.warmup} --ks {a.ks}" + (" --no-batch" if a.no_batch else "") + (" --no-ahead" if a.no_ahead else "") + (" --no-kernels" if a.no_kernels else ""),
             "", f"One process, the legs alternating; median (min .. max) of {a.runs} repetitions after {a.warmup}, host clock, ms. (a) = K sequential `prove` calls, the",
             "headline driver; (b) = K sequential reference-order proves" + ("." if a.no_batch else "; (c) = one `prove_batch` call over the same K states; (d) = (c) with")]
    if not a.no_batch:
        lines.append("`per_proof_opening=True`: the openings as K `sp_hyrax_prove` calls instead of one `sp_hyrax_prove_batch`.")
    if not a.no_batch and not a.no_options:
        lines.append("(g) = (c) with evals_rx + poly_ABC (`sp_poly_abc_batch`) and the rest commitments (one `sp_fixed_base_mul_h`) both forced to their batched forms; (e) = (g) with")
        lines.append("`per_proof_polyabc=True`; (f) = (g) with `per_proof_rest_commit=True`. A batched form becomes the driver's default from the smallest K at which the")
        lines.append("median of (g) lies below the minimum of (e), respectively (f).")
    if not a.no_batch and not a.no_ahead:
        lines.append("(h) = (c) with `opening_ahead=True`: the openings begun once comm_W is complete (`sp_hyrax_prove_batch_begin`), their row stage queued from the inner")
        lines.append("sum-check's hook (`_rows`) and collected by `_finish`; (i) = (c) with `opening_ahead=False`. The ahead form becomes the default from the smallest K at")
        lines.append("which the median of (h) lies below the minimum of (i).")
    names = [name for name, _ in legs]
    ratios = [] if a.no_batch else ["(c) / (a)", "(c) / (d)"]
    if "g" in names:
        ratios += ["(g) median < (e) min", "(g) median < (f) min"]
    if "h" in names:
        ratios += ["(h) median < (i) min"]
    cols = [f"({n}) total" for n in names] + [f"({n}) per proof" for n in names] + ratios
    lines += ["", "| K | " + " | ".join(cols) + " |", "|---|" + "---|" * len(cols)]
    phase_lines = []
    for K in ks:
        ts = {name: [] for name, _ in legs}
        ph = {name: [] for name, _ in legs}
        for rep in range(a.warmup + a.runs):
            for name, f in legs:
                t0 = time.perf_counter()
                phases = f(K)
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmup:
                    ts[name].append(dt)
                    ph[name].append(phases)
        s = {name: stat(v) for name, v in ts.items()}
        cells = [fmt(s[n]) for n in names] + [f"{s[n][0] / K:.3f}" for n in names]
        if ratios:
            cells += [f"{s['c'][0] / s['a'][0]:.2f}", f"{s['c'][0] / s['d'][0]:.2f}"]
        if "g" in s:
            cells += ["yes" if s["g"][0] < s["e"][1] else "no", "yes" if s["g"][0] < s["f"][1] else "no"]
        if "h" in s:
            cells += ["yes" if s["h"][0] < s["i"][1] else "no"]
        lines.append(f"| {K} | " + " | ".join(cells) + " |")
        print(lines[-1], flush=True)
        for name in ("c", "d", "e", "f", "g", "h", "i"):  # the batch's own phase split (wall-clock of the whole batch per phase), over the same repetitions
            if ph.get(name):
                phase_lines.append(f"| {K} | ({name}) | " + " | ".join(fmt(stat([p[k] for p in ph[name]])) for k in host.PHASES) + " |")
    if phase_lines:
        lines += ["", "Phases of the `prove_batch` calls above, ms for the whole batch, median (min .. max) over the same repetitions:", "",
                  "| K | leg | " + " | ".join(host.PHASES) + " |", "|---|---|" + "---|" * len(host.PHASES)] + phase_lines
    if not a.no_batch and not a.no_kernels:  # the batched opening's launches at the largest K, by the HIP events around them
        behind = {} if a.no_ahead else {"opening_ahead": False}
        batch(kmax, **behind)
        ctx.reset_stats(True)
        batch(kmax, **behind)
        ctx.synchronize()
        lines += ["", f"The launches of one `sp_hyrax_prove_batch` at K = {kmax} (HIP events around each launch):", "", "| kernel class | launches | device ms |", "|---|---|---|"]
        for what in ("opening_batch_mask", "opening_batch_rowmat", "opening_batch_walk", "opening_batch_z"):
            ms, launches, _ = ctx.kernel_stats(what)
            lines.append(f"| {what} | {launches} | {ms:.4f} |")
        if not a.no_ahead:
            batch(kmax, opening_ahead=True)
            ctx.reset_stats(True)
            batch(kmax, opening_ahead=True)
            ctx.synchronize()
            lines += ["", f"The launches of the same opening begun ahead (`opening_ahead=True`) at K = {kmax}, on the auxiliary stream beside the sum-checks' launches:", "",
                      "| kernel class | launches | device ms |", "|---|---|---|"]
            for what in ("opening_batch_dvec", "opening_batch_rowmat", "opening_batch_walk", "opening_batch_ip", "opening_batch_z"):
                ms, launches, _ = ctx.kernel_stats(what)
                lines.append(f"| {what} | {launches} | {ms:.4f} |")
        ctx.reset_stats(False)
    if not a.no_batch and not a.no_options and not a.no_kernels:
        poly_abc_launches(ctx, sn, lines, kmax)
    for ps, _ in states:
        host.lib().ss_prep_free(ps)
    if not a.no_batch and not a.no_kernels:
        kernels_alone(ctx, lines)
    sn.close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
