"""What NeutronNovaZkSNARK.verify_batch buys, timed on the device's host at the config-3 shape (32 sha256_step_circuit instances + the core circuit, one
key, one prepared state re-proved K times: every prove rerandomises, so these are distinct valid proofs): K proofs as (a) K sequential `verify` calls and
(b) one `verify_batch` call in its shared form (the step-instance folds of all proofs as one sp_msm_shared_weights_grouped, the matrix evaluations per
chunk of proofs, the transcript work per proof, one combined opening). One process, the legs alternating; median (min .. max) of `runs` repetitions after
`warmup`, host clock. The shared form becomes verify_batch's default from the smallest K at which the median of (b) lies below the minimum of (a)
(NN_VERIFY_BATCH_MIN in host/neutronnova_zk.cpp). Then the laps of ONE verify (SPARTAN_HOST_LAPS=1, read once per process: a child process of this
tool prints them), which name the sequential remainder, and the grouped commitment fold against G back-to-back sp_msm_shared_weights calls at the key's
fold shape, by the HIP events around each whole call (sp_ctx_kernel_stats classes msm_grouped_call / msm_shared_weights_call) and by the host clock,
with the grouped call's window Horner forced to the device and to host threads beside them (sp_msm_shared_weights_grouped_opts).
Writes a Markdown report (profiles/nn_verify_batch.md holds this output).
usage: python tools/nn_verify_batch_timing.py [--out FILE] [--runs 20] [--warmup 3] [--ks 1,4,16] [--gs 4,16] [--steps 32] [--no-laps] [--no-fold]"""
import argparse
import os
import statistics
import subprocess
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


def make_key(ctx, steps):
    circs = [frontend.sha256_step_circuit(bytes([i]) * 64) for i in range(steps)]
    core = frontend.sha256_step_circuit(bytes(64))
    nn = host.NeutronNovaZkSNARK(ctx, circs, core)
    tape = np.random.default_rng(0xC3).integers(0, 256, size=(65536, 64), dtype=np.uint8)
    return nn, tape, circs[0]


def laps_child(steps):
    """one key, one proof, three verify calls: with SPARTAN_HOST_LAPS=1 in the environment every call prints its laps to stderr"""
    ctx = hip.Context(0)
    nn, tape, _ = make_key(ctx, steps)
    used = nn.prep_prove(tape)
    proof, _, _ = nn.prove(tape[used:])
    for _ in range(3):
        sys.stderr.write("nn_verify call\n")
        assert nn.verify(proof) == 0
    nn.close()
    ctx.close()


def fold_comparison(ctx, lines, rows, n, gs, reps):
    pool = host.from_label(b"fold", rows * n).reshape(rows, n, 8)
    rng = np.random.default_rng(11)
    lines += ["", f"## The commitment fold alone: {rows} rows x {n} weights a group (the key's fold shape)", "",
              f"G groups as G back-to-back `sp_msm_shared_weights` calls and as one `sp_msm_shared_weights_grouped` call (chunks of {hip.msm_shared_weights_group_rows()} rows), the same",
              f"inputs, results compared; ms a batch of G groups, mean over {reps} repetitions, the forms alternating, the second round reported: HIP events around each whole call (first upload to last",
              "copy back, host-side tails included) and the host clock around the same calls. The last two columns: the grouped call with its window Horner forced to one",
              "device launch and to host threads (`sp_msm_shared_weights_grouped_opts`), by events: what `MSM_GROUP_HOST_HORNER_ROWS` in csrc/capi_group.hip is decided by.", "",
              "| G | rows in all | single calls, events | grouped, events | single calls, host | grouped, host | grouped / single (events) | grouped, Horner on the device | grouped, Horner on host threads |",
              "|---|---|---|---|---|---|---|---|---|"]
    for G in gs:
        w = rng.integers(0, 1 << 62, size=(G, n, 4), dtype=np.uint64)  # (canonical Montgomery limbs: the top limb stays below the modulus')
        bases = np.ascontiguousarray(np.broadcast_to(pool, (G, rows, n, 8)))

        def single():
            return [hip.msm_shared_weights(ctx, w[g], bases[g]) for g in range(G)]

        def grouped():
            return hip.msm_shared_weights_grouped(ctx, w, bases)

        def forced(side):
            return lambda: hip.msm_shared_weights_grouped(ctx, w, bases, horner=side)

        want = np.stack(single())
        assert all((f() == want).all() for f in (grouped, forced(hip.MSM_GROUPED_HORNER_HOST), forced(hip.MSM_GROUPED_HORNER_DEVICE)))
        res = {}
        for rnd in range(2):  # the four forms alternating, twice; the second round is reported
            for name, f, what in (("single", single, "msm_shared_weights_call"), ("grouped", grouped, "msm_grouped_call"),
                                  ("device", forced(hip.MSM_GROUPED_HORNER_DEVICE), "msm_grouped_call"), ("host", forced(hip.MSM_GROUPED_HORNER_HOST), "msm_grouped_call")):
                ctx.synchronize()
                ctx.reset_stats(True)
                t0 = time.perf_counter()
                for _ in range(reps):
                    f()
                host_ms = (time.perf_counter() - t0) * 1e3 / reps
                ctx.synchronize()
                ms, launches, _ = ctx.kernel_stats(what)
                # (below 64 rows in all the grouped entry point runs the single call per group: its time is then under the single call's class)
                if name != "single" and launches == 0:
                    ms, launches, _ = ctx.kernel_stats("msm_shared_weights_call")
                res[name] = (ms / reps, host_ms)
                ctx.reset_stats(False)
        lines.append(f"| {G} | {G * rows} | {res['single'][0]:.3f} | {res['grouped'][0]:.3f} | {res['single'][1]:.3f} | {res['grouped'][1]:.3f} | {res['grouped'][0] / res['single'][0]:.2f} | "
                     f"{res['device'][0]:.3f} | {res['host'][0]:.3f} |")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_verify_batch.md"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ks", default="1,4,16")
    ap.add_argument("--gs", default="4,16")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--no-laps", action="store_true")
    ap.add_argument("--no-fold", action="store_true")
    ap.add_argument("--laps-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.laps_child:
        laps_child(a.steps)
        return
    laps_lines = []
    if not a.no_laps:  # first, while this process has not opened the device: the child is a fresh process
        env = dict(os.environ, SPARTAN_HOST_LAPS="1")
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--laps-child", "--steps", str(a.steps)], env=env, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True,
                             timeout=300).stderr
        last = out.split("nn_verify call\n")[-1]
        laps_lines = ["", "## The laps of one `verify` (the third call of a fresh process with SPARTAN_HOST_LAPS=1; the fold and the matrix evaluations run beside them on the second context)", "",
                      "```"] + [ln for ln in last.splitlines() if ln.startswith(("nn_verify lap", "msm_shared_weights lap"))] + ["```"]
    ks = [int(k) for k in a.ks.split(",")]
    kmax = max(ks)
    ctx = hip.Context(0)
    nn, tape, step = make_key(ctx, a.steps)
    first = pos = nn.prep_prove(tape)
    proofs = []
    for _ in range(kmax):
        words, used, _ = nn.prove(tape[pos:])
        pos = pos + used if pos + 3 * used < tape.shape[0] else first + 1 + len(proofs)  # (a fresh stretch of the tape per proof, wrapping with an offset)
        proofs.append(words)
    assert all(not (proofs[0] == p).all() for p in proofs[1:])
    assert nn.verify_batch(proofs, per_proof=False) == [0] * kmax and all(nn.verify(p) == 0 for p in proofs)
    legs = [("a", lambda K: [nn.verify(p) for p in proofs[:K]]), ("b", lambda K: nn.verify_batch(proofs[:K], per_proof=False))]
    lines = [f"# NeutronNovaZkSNARK.verify_batch on the MI355X, config 3: {a.steps} sha256 step circuits + the core circuit, proofs of {len(proofs[0]) * 8} bytes", "",
             f"command: python tools/nn_verify_batch_timing.py --runs {a.runs} --warmup {a.warmup} --ks {a.ks} --gs {a.gs} --steps {a.steps}", "",
             f"One process, the legs alternating; median (min .. max) of {a.runs} repetitions after {a.warmup}, host clock, ms. (a) = K sequential `verify` calls; (b) = one",
             "`verify_batch` call over the same K proofs in its shared form (`per_proof=False`; a batch of one is `verify` itself). The shared form becomes the default from the",
             "smallest K at which the median of (b) lies below the minimum of (a).", "",
             "| K | (a) total | (b) total | (a) per proof | (b) per proof | (b) / (a) | (b) median < (a) min |", "|---|---|---|---|---|---|---|"]
    for K in ks:
        ts = {name: [] for name, _ in legs}
        for rep in range(a.warmup + a.runs):
            for name, f in legs:
                t0 = time.perf_counter()
                f(K)
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmup:
                    ts[name].append(dt)
        s = {name: stat(v) for name, v in ts.items()}
        lines.append(f"| {K} | {fmt(s['a'])} | {fmt(s['b'])} | {s['a'][0] / K:.3f} | {s['b'][0] / K:.3f} | {s['b'][0] / s['a'][0]:.2f} | {'yes' if s['b'][0] < s['a'][1] else 'no'} |")
        print(lines[-1], flush=True)
    codes, info = nn.verify_batch(proofs, info=True, per_proof=False)
    lines += ["", f"`verify_batch` of the {kmax} proofs reports {info}."]
    lines += laps_lines
    if not a.no_fold:
        _, dims = host.pad_shape(step)
        rows = (dims["num_shared"] + dims["num_precommitted"] + dims["num_rest"]) // 2048
        n = 2
        while n < a.steps:
            n *= 2
        fold_comparison(ctx, lines, rows, n, [int(g) for g in a.gs.split(",")], 10)
    nn.close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
