"""Two ways from a message to a prep state, timed on the device's host: (a) the frontend path - frontend.sha256_circuit(msg) (a full circuit synthesis) +
prep_prove, which uploads the witness as machine words - and (b) prep_prove_sha256, whose witness is generated on the device from a plan made once per
key. Medians of `runs` calls after `warmup`; beside (b) the witness phase of its prep_prove (prep_ms[0]: staging + launch + kernel + the wait for it),
the kernel's own time by HIP events, and the CPU evaluation of the plan (plan.eval). The NeutronNova case: `steps` step circuits + the core circuit.
Prints a Markdown table (profiles/sha256_witness.md is this output).
usage: python tools/witness_timing.py [runs] [warmup]"""
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


def kernel_ms(ctx, f, runs):
    """mean device time of the sha256_witness launches of `runs` calls of f, by the events attached to the dispatch"""
    ctx.stats_filter("sha256_witness")
    ctx.reset_stats(True)
    for _ in range(runs):
        f()
    ctx.synchronize()
    ms, n, _ = ctx.kernel_stats("sha256_witness")
    ctx.reset_stats(False)
    ctx.stats_filter("")
    return ms / max(n, 1)


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    ctx = hip.Context(0)
    tape = np.random.default_rng(1).integers(0, 256, size=(32768, 64), dtype=np.uint8)
    rng = np.random.default_rng(2)
    print(f"medians of {runs} runs after {warmup} warm-up calls, ms\n")
    print("| case | variables | (a) sha256_circuit | (a) prep_prove | (a) witness phase | (a) total | (b) prep_prove_sha256 | (b) witness phase | (b) kernel (HIP events) | plan.eval (CPU) | plan (once per key) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for n in (64, 1024, 2048):
        msg = rng.bytes(n)
        t0 = time.perf_counter()
        plan = frontend.sha256_witness_plan(n)
        plan_ms = (time.perf_counter() - t0) * 1e3
        sn = host.SpartanSNARK(ctx, frontend.sha256_circuit(bytes(n)))
        state = {}

        def synth():
            state["inst"] = frontend.sha256_circuit(msg)

        def prep_a():
            sn.inst = state["inst"]
            sn.prep_prove(tape)

        wit_a = []

        def both_a():
            synth()
            prep_a()
            wit_a.append(sn.prep_phases()["witness"])

        wit_b = []

        def prep_b():
            sn.prep_prove_sha256(msg, tape)
            wit_b.append(sn.prep_phases()["witness"])

        a_synth = med(synth, runs, warmup)
        a_prep = med(prep_a, runs, warmup)
        a_total = med(both_a, runs, warmup)
        b_prep = med(prep_b, runs, warmup)
        k_ms = kernel_ms(ctx, prep_b, runs)
        e_ms = med(lambda: plan.eval(msg), runs, warmup)
        print(f"| Spartan, {n} B | {plan.n_aux} | {a_synth:.3f} | {a_prep:.3f} | {statistics.median(wit_a[-runs:]):.3f} | {a_total:.3f} | {b_prep:.3f} | "
              f"{statistics.median(wit_b[warmup:warmup + runs]):.3f} | {k_ms:.4f} | {e_ms:.3f} | {plan_ms:.1f} |", flush=True)
        sn.close()
    steps_n = 32
    blocks = [rng.bytes(64) for _ in range(steps_n)]
    core = frontend.sha256_step_circuit(bytes(64))
    t0 = time.perf_counter()
    splan = frontend.sha256_step_witness_plan()
    plan_ms = (time.perf_counter() - t0) * 1e3
    nn = host.NeutronNovaZkSNARK(ctx, [frontend.sha256_step_circuit(bytes([i]) * 64) for i in range(steps_n)], core)
    state = {}

    def synth():
        state["steps"] = [frontend.sha256_step_circuit(b) for b in blocks]
        state["core"] = frontend.sha256_step_circuit(bytes(64))

    def prep_a():
        nn.steps, nn.core = state["steps"], state["core"]
        nn.prep_prove(tape)

    def both_a():
        synth()
        prep_a()

    def prep_b():
        nn.prep_prove_sha256(blocks, tape)

    a_synth = med(synth, runs, warmup)
    a_prep = med(prep_a, runs, warmup)
    a_total = med(both_a, runs, warmup)
    b_prep = med(prep_b, runs, warmup)
    k_ms = kernel_ms(ctx, prep_b, runs)
    e_ms = med(lambda: [splan.eval(b) for b in blocks + [bytes(64)]], runs, warmup)
    print(f"| NeutronNova, {steps_n} steps + core | {steps_n + 1} x {splan.n_aux} | {a_synth:.3f} | {a_prep:.3f} | - | {a_total:.3f} | {b_prep:.3f} | - | {k_ms:.4f} | {e_ms:.3f} | {plan_ms:.1f} |",
          flush=True)
    nn.close()
    ctx.close()


if __name__ == "__main__":
    main()
