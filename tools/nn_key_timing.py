"""What loading NeutronNova keys from their bytes costs, timed on the device's host at config 3: the bench's 32 SHA-256 step circuits plus the core circuit
(2^15 constraints each - about 1/32 of config 2's shape, twice). One process per run of this tool. The size of both keys' bytes; NeutronNovaZkSNARK(ctx,
steps, core) - setup - as the reference point; NeutronNovaVerifier.from_bytes with the device and the host row decode, alternating call by call, and
NeutronNovaProver.from_bytes with SP_SHAPE_WIRE_FULL_DEVICE and SP_SHAPE_WIRE_FULL, each with the digest hashed and trusted, alternating: the whole call
(host clock around a call that returns synchronised) and the loader's stages (host clock inside the driver); the device memory each key holds (free memory
before and after, this process only); verify and prove on a loaded key against setup's key, alternating. Median and min .. max of `runs` repetitions after
`warmup`. The default form of each loader is stated from these figures by the rule of profiles/verifier_key.md: the device form only if its median lies
below the host form's minimum.
usage: python tools/nn_key_timing.py [--out profiles/nn_keys.md] [--runs 10] [--warmup 2] [--steps 32]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spartan2_amd import frontend, hip, host  # noqa: E402


def fmt(xs, unit=""):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f}){unit}"


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def free_bytes(ctx):
    ctx.synchronize()
    return torch.cuda.mem_get_info()[0]


STAGES = (("total", "the loader (nnz_*_from_bytes)"), ("hyrax_key", "ck read (2049 on-curve checks; a verifier's vk_ee compared)"), ("S_step", "sp_shape_from_wire: S_step"),
          ("S_core", "sp_shape_from_wire: S_core"), ("vc_shapes", "verifier circuit rebuilt, its two shapes compared; vc_ck read"), ("ck_create", "the two sp_ck_create"),
          ("digest", "digest (SHA-256 over the bytes, helper thread)"), ("digest_wait", "wait for the digest behind the rest"))


def table(lines, heads, cols):
    """cols: per column (whole-call ms, load_stages dicts)"""
    lines += ["| stage | " + " | ".join(heads) + " |", "|---" * (len(heads) + 1) + "|",
              "| whole call (host clock, Python included) | " + " | ".join(fmt(t) for t, _ in cols) + " |"]
    for key, label in STAGES:
        lines.append(f"| {label} | " + " | ".join(fmt([s[key] for s in st]) for _, st in cols) + " |")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_keys.md"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=32)
    a = ap.parse_args()
    assert a.runs >= 10, "at least 10 loads"
    runs, warmup, n = a.runs, a.warmup, a.steps
    ctx = hip.Context(0)
    blocks = [bytes([i]) * 64 for i in range(n)]
    steps = [frontend.sha256_step_circuit(b) for b in blocks]
    core = frontend.sha256_step_circuit(bytes(64))
    setup_ms, gnn = [], None
    for _ in range(3):
        if gnn is not None:
            gnn.close()
        ms, gnn = timed(lambda: host.NeutronNovaZkSNARK(ctx, steps, core))
        setup_ms.append(ms)
    vkb, pkb = gnn.vk_to_bytes(), gnn.pk_to_bytes()
    s_step, s_core = host.nn_key_shapes(gnn)
    nnz = [sum(s.info()["nnz"]) for s in (s_step, s_core)]
    lines = ["# NeutronNova keys loaded from their bytes, on the MI355X", "",
             "Written by tools/nn_key_timing.py: one process, host clock around calls that return synchronised and inside the loader.", "",
             f"## Config 3: {n} SHA-256 step circuits + the core circuit, {s_step.dims['num_cons']} constraints each, {nnz[0]} + {nnz[1]} entries in A, B, C of S_step + S_core", "",
             f"Verifier key: {len(vkb)} bytes ({len(vkb) / 2**20:.1f} MiB); prover key: {len(pkb)} bytes ({len(pkb) / 2**20:.1f} MiB). "
             f"`NeutronNovaZkSNARK(ctx, steps, core)` (setup, 3 calls): {fmt(setup_ms, ' ms')}.", ""]
    # the verifier's load
    vt = {True: ([], []), False: ([], [])}
    for i in range(warmup + runs):
        for device in (True, False):
            ms, v = timed(lambda: host.NeutronNovaVerifier.from_bytes(ctx, vkb, n, device_decode=device))
            assert v.vk_digest.tobytes() == gnn.vk_digest.tobytes() and v.wire_stages["device"] == float(device)
            if i >= warmup:
                vt[device][0].append(ms)
                vt[device][1].append(v.load_stages)
            v.close()
    lines += [f"`NeutronNovaVerifier.from_bytes`, the two row decodes alternating, {runs} loads each after {warmup}; ms, median (min .. max):", ""]
    table(lines, ["device decode", "host decode"], [vt[True], vt[False]])
    # the prover's load
    combos = [(True, False), (False, False), (True, True), (False, True)]  # (full_device, trust_digest)
    pt = {c: ([], []) for c in combos}
    for i in range(warmup + runs):
        for c in combos:
            ms, p = timed(lambda: host.NeutronNovaProver.from_bytes(ctx, pkb, n, full_device=c[0], trust_digest=c[1]))
            assert p.vk_digest.tobytes() == gnn.vk_digest.tobytes() and p.wire_stages["device"] == float(c[0])
            if i >= warmup:
                pt[c][0].append(ms)
                pt[c][1].append(p.load_stages)
            p.close()
    lines += [f"`NeutronNovaProver.from_bytes`, the four forms alternating, {runs} loads each after {warmup}; ms, median (min .. max):", ""]
    table(lines, ["FULL_DEVICE, digest hashed", "FULL (host), digest hashed", "FULL_DEVICE, digest trusted", "FULL (host), digest trusted"], [pt[c] for c in combos])
    # device memory
    gnn.close()
    held = {}
    for name, make in (("verifier", lambda: host.NeutronNovaVerifier.from_bytes(ctx, vkb, n)), ("prover", lambda: host.NeutronNovaProver.from_bytes(ctx, pkb, n)),
                       ("setup", lambda: host.NeutronNovaZkSNARK(ctx, steps, core))):
        base = free_bytes(ctx)
        k = make()
        held[name] = base - free_bytes(ctx)
        k.close()
    lines += ["Device memory (free memory before and after, this process): the loaded verifier key holds " f"{held['verifier'] / 2**20:.1f} MiB, the loaded prover key "
              f"{held['prover'] / 2**20:.1f} MiB, setup's key {held['setup'] / 2**20:.1f} MiB (each before a first verify or prep_prove allocates its tables).", ""]
    # verify and prove on loaded keys against setup's
    gnn = host.NeutronNovaZkSNARK(ctx, steps, core)
    pr = host.NeutronNovaProver.from_bytes(ctx, pkb, n)
    v = host.NeutronNovaVerifier.from_bytes(ctx, vkb, n)
    tape = np.random.default_rng(1).integers(0, 256, size=(65536, 64), dtype=np.uint8)
    # Two passes with fresh prep states, the order of first use swapped: a state's first prove and a key's first verify each create a second context on the
    # GPU for their side jobs, and a prove's time was seen to follow the order of first use, not the key (see the note below the table)
    rows = []
    for first in ("setup", "loaded"):
        objs = [("setup", gnn, gnn), ("loaded", v, pr)]
        if first == "loaded":
            objs.reverse()
        for _, _, po in objs:
            at = po.prep_prove_sha256(blocks, tape)
        words, _, _ = objs[0][2].prove(tape[at:])
        t = {k: [] for k in (("verify", "loaded"), ("verify", "setup"), ("prove", "loaded"), ("prove", "setup"))}
        for i in range(warmup + runs):
            for name, vo, po in objs:
                ms, rc = timed(lambda: vo.verify(words))
                assert rc == 0
                msp, out = timed(lambda: po.prove(tape[at:]))
                if i >= warmup:
                    t[("verify", name)].append(ms)
                    t[("prove", name)].append(msp)
        assert v.verify(pr.prove(tape[at:])[0]) == 0 and gnn.verify(pr.prove(tape[at:])[0]) == 0
        rows.append((first, t))
    lines += [f"verify and prove on a loaded key against setup's key (the same code; alternating, {runs} repetitions; whole call, host clock), ms:", "",
              "| first used | call | loaded key | setup's key | loaded median against setup's maximum |", "|---|---|---|---|---|"]
    for first, t in rows:
        for what in ("verify", "prove"):
            x, y = t[(what, "loaded")], t[(what, "setup")]
            lines.append(f"| {first} | {what} | {fmt(x)} | {fmt(y)} | {'within' if statistics.median(x) <= max(y) else 'EXCEEDS'} |")
    lines += ["", "The passes differ in which object proves first: a state's first prove creates a second context on the GPU for the side jobs of its proves, and a prove's "
              "time has been seen to depend on that order (two levels about 0.7 ms apart, in the NIFS and outer sum-check phases) and not on where the key came from - "
              "hence two passes; a key is slower than the other only if it is so in both.", ""]
    for o in (v, pr, gnn):
        o.close()
    ctx.close()
    # the defaults
    L = host.lib()
    lines += ["## The default decode forms", ""]
    for who, dev, hst, default, names in (("NeutronNovaVerifier.from_bytes", vt[True][1], vt[False][1], bool(L.nnz_verifier_device_default()), ("device row decode", "host row decode")),
                                          ("NeutronNovaProver.from_bytes (digest hashed)", pt[(True, False)][1], pt[(False, False)][1], bool(L.nnz_prover_full_device_default()),
                                           ("FULL_DEVICE", "FULL (host)"))):
        dev_med, host_min = statistics.median(s["total"] for s in dev), min(s["total"] for s in hst)
        wins = dev_med < host_min
        lines += [f"{who}: {names[0]}, median {dev_med:.3f} ms; {names[1]}, minimum {host_min:.3f} ms; setup, median {statistics.median(setup_ms):.3f} ms. "
                  + (f"The device form's median lies below the host form's minimum: {names[0]} is the default." if wins else
                     f"The device form's median does NOT lie below the host form's minimum: it was measured and did not win; {names[1]} is the default and the device form stays "
                     "reachable by flag.") + f" The library's default in this run: {names[0] if default else names[1]}" + ("." if default == wins else " - NOT what this run's rule gives.")]
    lines.append("")
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
