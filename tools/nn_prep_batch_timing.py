"""What NeutronNovaZkSNARK.prep_prove_batch costs, timed on the device's host at the config-3 key (32 SHA-256 steps + core, 2^15 variables a circuit):
K prep states as (a) K sequential prep_prove_sha256 calls (`one_pass=False`, the loop - the code path there was before the batch), (b) one one-pass
call with BOTH shared stages (sp_hyrax_commit_batch, sp_nifs_layers_batch), (c) (b) with per_state_commit (one sp_hyrax_commit per polynomial),
(d) (b) with per_state_layers (nifs_prepare per state). One process, the legs alternating; median (min .. max) of `runs` repetitions after `warmup`,
host clock, every leg ending in a device synchronise; the states of the repetition before are freed outside the timed region. Then the phases of the
one-pass calls, the rule that picks the driver's defaults applied to the table, the kernels by HIP events, and one state of each leg proven with the
same tape: the proof words must be equal. Writes a Markdown report (profiles/nn_prep_prove_batch.md holds this output).
usage: python tools/nn_prep_batch_timing.py [--out FILE] [--runs 12] [--warmup 3] [--ks 1,4,16] [--steps 32] [--no-kernels]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spartan2_amd import frontend, hip, host  # noqa: E402

PHASE_NAMES = ("blinds_alloc", "witness", "commit", "layers", "mirrors", "sync", "total")
SHARED = dict(shared_commit=True, shared_layers=True)
LEGS = [("a", dict(one_pass=False)), ("b", dict(SHARED)), ("c", dict(SHARED, per_state_commit=True)), ("d", dict(SHARED, per_state_layers=True))]


def stat(ts):
    return statistics.median(ts), min(ts), max(ts)


def fmt(s):
    return f"{s[0]:.3f} ({s[1]:.3f} .. {s[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_prep_prove_batch.md"))
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ks", default="1,4,16")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--no-kernels", action="store_true")
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
    prove_tape = np.random.default_rng(200).integers(0, 256, size=(8192, 64), dtype=np.uint8)

    def prep(K, **kw):
        nn._free_batch()
        ctx.synchronize()
        t0 = time.perf_counter()
        nn.prep_prove_batch(prep_tapes[:K], blocks=blocks[:K], **kw)
        ctx.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        return dt, (dict(nn.batch_prep_phases) if kw.get("one_pass", True) else None)

    lines = [f"# NeutronNovaZkSNARK.prep_prove_batch on the MI355X: {n} SHA-256 steps + core, {steps[0].num_cons} constraints a circuit", "",
             f"command: python tools/nn_prep_batch_timing.py --runs {a.runs} --warmup {a.warmup} --ks {a.ks} --steps {n}" + (" --no-kernels" if a.no_kernels else ""), "",
             f"One process, the legs alternating; median (min .. max) of {a.runs} repetitions after {a.warmup}, host clock around a call that ends in a device",
             "synchronise, ms. (a) = K sequential `prep_prove_sha256` calls (the loop, `one_pass=False`: the code path from before the batch, the comparison",
             "base); (b) = one one-pass `prep_prove_batch` call with both shared stages (`sp_hyrax_commit_batch`, `sp_nifs_layers_batch`); (c) = (b) with",
             "`per_state_commit=True`: one `sp_hyrax_commit` per polynomial; (d) = (b) with `per_state_layers=True`: `nifs_prepare` per state. The states of",
             "the repetition before are freed outside the timed region."]
    names = [nm for nm, _ in LEGS]
    cols = [f"({nm}) total" for nm in names] + [f"({nm}) per state" for nm in names] + ["(b) / (a)", "(b) / (c)", "(b) / (d)"]
    lines += ["", "| K | " + " | ".join(cols) + " |", "|---|" + "---|" * len(cols)]
    phase_lines, rule_lines = [], []
    for K in ks:
        ts = {nm: [] for nm in names}
        ph = {nm: [] for nm in names}
        for rep in range(a.warmup + a.runs):
            for nm, kw in LEGS:
                dt, phases = prep(K, **kw)
                if rep >= a.warmup:
                    ts[nm].append(dt)
                    if phases:
                        ph[nm].append(phases)
        s = {nm: stat(v) for nm, v in ts.items()}
        cells = [fmt(s[nm]) for nm in names] + [f"{s[nm][0] / K:.3f}" for nm in names] + [f"{s['b'][0] / s[o][0]:.2f}" for o in ("a", "c", "d")]
        lines.append(f"| {K} | " + " | ".join(cells) + " |")
        print(lines[-1], flush=True)
        for nm in ("b", "c", "d"):
            phase_lines.append(f"| {K} | ({nm}) | " + " | ".join(fmt(stat([p[k] for p in ph[nm]])) for k in PHASE_NAMES) + " |")
        # the rule: a shared stage is the default only where (b)'s median is below the minimum of the leg that takes the per-state form of that stage
        for stage, other in (("commit (`sp_hyrax_commit_batch`)", "c"), ("layers (`sp_nifs_layers_batch`)", "d")):
            wins = s["b"][0] < s[other][1]
            rule_lines.append(f"| {K} | {stage} | {s['b'][0]:.3f} | ({other}) {s[other][1]:.3f} | {'shared' if wins else 'per state'} |")
    lines += ["", "Phases of the one-pass calls above, ms for the whole batch (host clock between the phases; `sp_nifs_prepare_small` waits for the layers it reads, so",
              "device time of the layers kernel that is still queued when `layers` ends is counted in `mirrors`), median (min .. max) over the same repetitions:", "",
              "| K | leg | " + " | ".join(PHASE_NAMES) + " |", "|---|---|" + "---|" * len(PHASE_NAMES)] + phase_lines
    lines += ["", "## The rule for the driver's defaults", "",
              "A shared stage is the driver's default only where the median of (b) is below the MINIMUM of the leg that runs the per-state form of that stage:", "",
              "| K | stage | (b) median | per-state leg, minimum | the rule says |", "|---|---|---|---|---|"] + rule_lines
    all_shared = all(ln.endswith("| shared |") for ln in rule_lines)
    lines += ["", ("The shared form wins both stages at every K measured: the driver takes both from one state on (`NN_PREP_SHARED_COMMIT_MIN` = `NN_PREP_SHARED_LAYERS_MIN` = 1,"
                   " `host/neutronnova_zk.cpp`); the per-state forms run on request." if all_shared else
                   "Where the rule says `per state`, that form stays the driver's default at that K (`NN_PREP_SHARED_*_MIN`, `host/neutronnova_zk.cpp`) and the shared stage runs on request.")]
    nn._free_batch()

    if not a.no_kernels:  # the launches of one state and of one batch, by the HIP events around them
        classes = ("sha256_witness", "commit_canon_classify", "msm_binary_rows", "fixed_base", "spmv", "nifs_layers", "nifs_to_small")
        for title, K, kw in (("one state (`prep_prove_sha256`)", 1, dict(one_pass=False)), (f"one batch, K = {kmax}, both stages shared", kmax, dict(SHARED)),
                             (f"K = {kmax} with `per_state_commit` and `per_state_layers`", kmax, dict(per_state_commit=True, per_state_layers=True))):
            prep(K, **kw)
            nn._free_batch()
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
            nn._free_batch()

    # one state of each leg, proven with the same tape: the same proof words
    K = min(kmax, 4)
    words = {}
    for nm, kw in LEGS + [("default", dict())]:
        prep(K, **kw)
        words[nm], _, _ = nn.prove(prove_tape, state=K - 1)
        assert nn.verify(words[nm]) == 0, f"leg ({nm}): the proof of state {K - 1} is rejected"
    same = all((words[nm] == words["a"]).all() for nm in words)
    lines += ["", f"State {K - 1} of a batch of {K} from every leg and from the driver's default, proven with one tape: proof words "
              + ("EQUAL across (a), (b), (c), (d) and the default, and accepted by `verify`." if same else "DIFFER - the legs do not make the same state.")]
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
