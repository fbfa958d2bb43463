"""What NeutronNovaZkSNARK.prove_batch costs, timed on the device's host at the config-3 key (32 SHA-256 steps + core): K prepared states proven as
(a) K sequential prove() calls (the code path there was before the batch: the yardstick), (b) prove_batch forced per proof (per_proof=True: the same
loop inside one call), (c) prove_batch forced lockstep (per_proof=False: the batched outer and inner sum-checks of all K proofs one launch a round).
One process, the legs alternating; median (min .. max) of `runs` repetitions after `warmup`, host clock, every leg ending in a device synchronise.
Then the phases of the lockstep batch, the rule that picks the driver's default applied to the table, the per-round cost of the two lockstep calls
against K single calls at the key's table sizes (a trivial hook), and the proofs of every leg compared word for word. Writes a Markdown report
(profiles/nn_prove_batch.md holds this output).
usage: python tools/nn_prove_batch_timing.py [--out FILE] [--runs 20] [--warmup 3] [--ks 1,2,4,8,16] [--steps 32]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spartan2_amd import frontend, hip, host  # noqa: E402


def stat(ts):
    return statistics.median(ts), min(ts), max(ts)


def fmt(s):
    return f"{s[0]:.3f} ({s[1]:.3f} .. {s[2]:.3f})"


def rand_table(rng, n):
    """n field elements below 2^248 in Montgomery-agnostic limbs (any canonical value serves a timing run)"""
    t = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    t[:, 3] >>= np.uint64(8)
    return t


def per_round(ctx, rng, nx, ny, ks, runs, warmup):
    """ms per round of one lockstep call over K pairs against K single calls, trivial hooks, tables of the key's sizes"""
    hook = lambda rnd, cs, cc: cs[0]
    rows = []
    for K in ks:
        res = {}
        for kind, nr in (("outer", nx), ("inner", ny)):
            n = 1 << nr
            left = 1 << (nr // 2)
            right = n // left
            src = [rand_table(rng, n) for _ in range(6)]
            pls, prs = [hip.Table.from_host(ctx, rand_table(rng, left)) for _ in range(K)], [hip.Table.from_host(ctx, rand_table(rng, right)) for _ in range(K)]
            tabs = [[hip.Table.zeros(ctx, n) for _ in range(6)] for _ in range(K)]

            def fill():
                for ts in tabs:
                    for t, s in zip(ts, src):
                        t.write(0, s)
                        t.set_len(n)
                ctx.synchronize()

            single, lock = [], []
            for rep in range(warmup + runs):
                for leg in ("single", "lockstep"):
                    fill()
                    t0 = time.perf_counter()
                    if kind == "outer":
                        if leg == "single":
                            for k in range(K):
                                hip.sumcheck_cubic_outer_pow_batched(ctx, nr, pls[k], prs[k], tabs[k][:3], tabs[k][3:], src[0][0], 0, hook)
                        else:
                            hip.sumcheck_cubic_outer_pow_batched_lockstep(ctx, nr, pls, prs, [t[:3] for t in tabs], [t[3:] for t in tabs], np.stack([src[0][0]] * K), 0, [hook] * K)
                    else:
                        if leg == "single":
                            for k in range(K):
                                hip.sumcheck_quad_batched(ctx, src[0][:2], nr, *tabs[k][:4], 0, hook)
                        else:
                            hip.sumcheck_quad_batched_lockstep(ctx, np.stack([src[0][:2]] * K), nr, *[[t[m] for t in tabs] for m in range(4)], 0, [hook] * K)
                    ctx.synchronize()
                    if rep >= warmup:
                        (single if leg == "single" else lock).append((time.perf_counter() - t0) * 1e3 / nr)
            res[kind] = (stat(single), stat(lock))
        rows.append(f"| {K} | {fmt(res['outer'][0])} | {fmt(res['outer'][1])} | {res['outer'][1][0] / res['outer'][0][0]:.2f} | {fmt(res['inner'][0])} | {fmt(res['inner'][1])} | "
                    f"{res['inner'][1][0] / res['inner'][0][0]:.2f} |")
        print(rows[-1], flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_prove_batch.md"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--steps", type=int, default=32)
    a = ap.parse_args()
    if a.runs < 10:
        ap.error("at least 10 repetitions")
    ks = [int(k) for k in a.ks.split(",")]
    kmax, n = max(ks), a.steps
    ctx = hip.Context(0)
    steps = [frontend.sha256_step_circuit(bytes([i]) * 64) for i in range(n)]
    nn = host.NeutronNovaZkSNARK(ctx, steps, frontend.sha256_step_circuit(bytes(64)))
    rng = np.random.default_rng(3)
    blocks = [[rng.bytes(64) for _ in range(n)] for _ in range(kmax)]
    prep_tapes = [np.random.default_rng(100 + k).integers(0, 256, size=(1024, 64), dtype=np.uint8) for k in range(kmax)]
    tapes = [np.random.default_rng(200 + k).integers(0, 256, size=(8192, 64), dtype=np.uint8) for k in range(kmax)]
    nn.prep_prove_batch(prep_tapes, blocks=blocks)
    ctx.synchronize()

    def leg_a(K):
        return [nn.prove(tapes[k], state=k)[0] for k in range(K)]

    def leg_b(K):
        return [w for w, _ in nn.prove_batch(tapes[:K], states=list(range(K)), per_proof=True)]

    def leg_c(K):
        return [w for w, _ in nn.prove_batch(tapes[:K], states=list(range(K)), per_proof=False)]

    legs = [("a", leg_a), ("b", leg_b), ("c", leg_c)]
    lines = [f"# NeutronNovaZkSNARK.prove_batch on the MI355X: {n} SHA-256 steps + core, {steps[0].num_cons} constraints a circuit", "",
             f"command: python tools/nn_prove_batch_timing.py --runs {a.runs} --warmup {a.warmup} --ks {a.ks} --steps {n}", "",
             f"One process, the legs alternating; median (min .. max) of {a.runs} repetitions after {a.warmup}, host clock around calls that end in a device",
             "synchronise, ms. K prepared states (`prep_prove_batch`, outside the timed region), each proven with its own tape. (a) = K sequential `prove(tape,",
             "state=k)` calls: unchanged code, the yardstick; (b) = `prove_batch(per_proof=True)`: the same loop inside one call; (c) =",
             "`prove_batch(per_proof=False)`: the batched outer and inner sum-checks of all K proofs in lockstep, everything else per proof.", "",
             "| K | (a) total | (b) total | (c) total | (a) per proof | (b) per proof | (c) per proof | (c) / (a) |", "|---|---|---|---|---|---|---|---|"]
    phase_lines, rule_lines, first_k, same = [], [], None, True
    for K in ks:
        ts = {nm: [] for nm, _ in legs}
        ph = []
        for rep in range(a.warmup + a.runs):
            for nm, fn in legs:
                ctx.synchronize()
                t0 = time.perf_counter()
                words = fn(K)
                ctx.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmup:
                    ts[nm].append(dt)
                    if nm == "c":
                        ph.append(dict(nn.batch_prove_phases))
                if rep == 0:
                    if nm == "a":
                        want = words
                    else:
                        same = same and all((w == v).all() for w, v in zip(words, want))
        s = {nm: stat(v) for nm, v in ts.items()}
        lines.append(f"| {K} | {fmt(s['a'])} | {fmt(s['b'])} | {fmt(s['c'])} | {s['a'][0] / K:.3f} | {s['b'][0] / K:.3f} | {s['c'][0] / K:.3f} | {s['c'][0] / s['a'][0]:.2f} |")
        print(lines[-1], flush=True)
        phase_lines.append(f"| {K} | " + " | ".join(fmt(stat([p[k] for p in ph])) for k in host.NN_BATCH_PROVE_PHASES[:-1]) + " |")
        wins = s["c"][0] < s["a"][1]
        if wins and first_k is None:
            first_k = K
        rule_lines.append(f"| {K} | {s['c'][0]:.3f} | {s['a'][1]:.3f} | {'lockstep' if wins else 'per proof'} |")
    lines += ["", "Phases of the lockstep batch (c) above, ms for the whole batch (host clock between the phases), median (min .. max) over the same repetitions. head =",
              "setup .. NIFS per proof; outer / inner before, sum-check (ONE lockstep call), after; tail = verifier-circuit instance .. emit per proof:", "",
              "| K | " + " | ".join(host.NN_BATCH_PROVE_PHASES[:-1]) + " |", "|---|" + "---|" * (len(host.NN_BATCH_PROVE_PHASES) - 1)] + phase_lines
    lines += ["", "## The rule for the driver's default", "",
              "Lockstep is the driver's default from the smallest K at which the median of (c) lies below the MINIMUM of (a); below it the driver loops over `nn_prove`:", "",
              "| K | (c) median | (a) minimum | the rule says |", "|---|---|---|---|"] + rule_lines
    lines += ["", (f"The smallest such K measured is {first_k}: `NN_PROVE_BATCH_LOCKSTEP_MIN` (`host/neutronnova_zk.cpp`) is set from this table." if first_k is not None else
                   "No K measured qualifies: the lockstep form is NOT the default at any batch size (`NN_PROVE_BATCH_LOCKSTEP_MIN` = never, `host/neutronnova_zk.cpp`); it runs on request only (`per_proof=False`, `NNZ_BATCH_LOCKSTEP`).")]
    nx, ny = nn.info["nx"], nn.info["ny"]
    nn._free_batch()
    lines += ["", "## The two lockstep calls against K single calls, per round", "",
              f"`sp_sumcheck_cubic_outer_pow_batched_lockstep` over K pairs of 2^{nx}-entry tables against K `sp_sumcheck_cubic_outer_pow_batched` calls, and",
              f"`sp_sumcheck_quad_batched_lockstep` over K pairs of 2^{ny}-entry tables against K `sp_sumcheck_quad_batched` calls: ms per ROUND for all K pairs (the call's",
              "time over its rounds), trivial Python hooks on both sides (their cost, K hooks a round, is in both columns), dense tables:", "",
              "| K | outer: K single calls | outer: lockstep | ratio | inner: K single calls | inner: lockstep | ratio |", "|---|---|---|---|---|---|---|"]
    lines += per_round(ctx, rng, nx, ny, ks, a.runs, a.warmup)
    lines += ["", "Proof words of (b) and (c) against (a), every proof of every K: " + ("EQUAL." if same else "DIFFER.")]
    nn.close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
