"""What loading a verifier key from its bytes costs, timed on the device's host: the config-2 key (sha256_circuit(bytes(2048)): 2^20 constraints) and
the 64-byte key (2^16). One process per run of this tool. Per key: the size of the bytes and the entry count; SpartanSNARK(ctx, inst) - setup - as the
reference point; SpartanVerifier.from_bytes with the device decode and with the host decode, alternating call by call: the whole call (host clock around a
call that returns synchronised) and its stages - the Hyrax keys read, the shape, the two sp_ck_create, the digest on its helper thread (host clock inside
the driver) and, inside the shape's device decode, upload / entry kernel / counts + scan / scatter (HIP events on the context's stream); the device memory
a loaded key and a prover's key hold (free memory before and after, this process only); verify and verify_batch(K = 16) on the loaded key against the
prover's key, alternating. Median and min .. max of `runs` repetitions after `warmup`. The decision between the two decode forms is stated from the
config-2 figures: the device form is the default only if its median lies below the host form's minimum. --bench takes JSON lines of
`python bench.py --gpus 1 --steps 20 --warmup 3` runs (label=path, repeated) for the prove-is-unchanged table.
usage: python tools/verifier_key_timing.py [--out profiles/verifier_key.md] [--runs 10] [--warmup 2] [--bench this1=a.json --bench parent1=b.json ...]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spartan2_amd import frontend, hip, host  # noqa: E402

K_BATCH = 16


def fmt(xs, unit=""):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f}){unit}"


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def free_bytes(ctx):
    ctx.synchronize()
    return torch.cuda.mem_get_info()[0]


def make_proofs(sn, n, msg_len):
    rng = np.random.default_rng(7)
    tape = np.random.default_rng(1).integers(0, 256, size=(8192, 64), dtype=np.uint8)
    proofs = []
    for _ in range(n):
        used = sn.prep_prove_sha256(rng.bytes(msg_len), tape)
        proofs.append(sn.prove(tape[used:])[0])
    return proofs


def one_key(ctx, msg_len, runs, warmup, lines):
    inst = frontend.sha256_circuit(bytes(msg_len))
    setup_ms = []
    sn = None
    for _ in range(3):
        if sn is not None:
            sn.close()
        ms, sn = timed(lambda: host.SpartanSNARK(ctx, inst))
        setup_ms.append(ms)
    vk = sn.vk_to_bytes()
    nnz = sum(sn.shape_info["nnz"])
    lines += [f"## {msg_len}-byte messages: {sn.dims['num_cons']} constraints, {nnz} entries in A, B, C", "",
              f"Key: {len(vk)} bytes ({len(vk) / 2**20:.1f} MiB; 40 bytes an entry = {40 * nnz} of them). `SpartanSNARK(ctx, inst)` (setup, 3 calls): {fmt(setup_ms, ' ms')}.", ""]
    total = {True: [], False: []}
    load = {True: [], False: []}
    dec = {True: [], False: []}
    for i in range(warmup + runs):
        for device in (True, False):
            ms, v = timed(lambda: host.SpartanVerifier.from_bytes(ctx, vk, device_decode=device, timed=True))
            assert v.vk_digest.tobytes() == sn.vk_digest.tobytes() and v.stages["device"] == float(device)
            if i >= warmup:
                total[device].append(ms)
                load[device].append(v.load_stages)
                dec[device].append(v.stages)
            v.close()
    lines += [f"`SpartanVerifier.from_bytes`, the two decode forms alternating, {runs} loads each after {warmup}; ms, median (min .. max):", "",
              "| stage | device decode | host decode |", "|---|---|---|",
              f"| whole call (host clock, Python included) | {fmt(total[True])} | {fmt(total[False])} |"]
    for key, label in (("total", "ss_verifier_from_bytes"), ("hyrax_keys", "the two Hyrax keys read (2049 + 2 on-curve checks)"), ("shape", "sp_shape_from_wire"),
                       ("ck_create", "the two sp_ck_create"), ("digest", "digest (SHA-256 over the bytes, helper thread)"), ("digest_wait", "wait for the digest behind the rest")):
        lines.append(f"| {label} | {fmt([s[key] for s in load[True]])} | {fmt([s[key] for s in load[False]])} |")
    for key, label in (("parse", "sp_shape_from_wire: parse + checks (host, O(rows))"), ("decode", "sp_shape_from_wire: decode")):
        lines.append(f"| {label} | {fmt([s[key] for s in dec[True]])} | {fmt([s[key] for s in dec[False]])} |")
    for key, label in (("upload", "device decode: upload of the raw bytes"), ("entries", "device decode: k_wire_entries"), ("counts_scan", "device decode: k_wire_row_counts + scan"),
                       ("scatter", "device decode: totals read back, allocations, k_wire_scatter")):
        lines.append(f"| {label} (HIP events) | {fmt([s[key] for s in dec[True]])} | - |")
    lines.append("")
    # device memory
    sn.close()
    base = free_bytes(ctx)
    v = host.SpartanVerifier.from_bytes(ctx, vk)
    held_v = base - free_bytes(ctx)
    v.close()
    base = free_bytes(ctx)
    sn = host.SpartanSNARK(ctx, inst)
    held_p = base - free_bytes(ctx)
    lines += [f"Device memory (free memory before and after, this process): the loaded key holds {held_v / 2**20:.1f} MiB, the prover's key {held_p / 2**20:.1f} MiB "
              "(both before a first verify allocates its tables).", ""]
    # verify on both keys
    proofs = make_proofs(sn, K_BATCH, msg_len)
    v = host.SpartanVerifier.from_bytes(ctx, vk)
    t = {("verify", "loaded"): [], ("verify", "prover"): [], ("batch", "loaded"): [], ("batch", "prover"): []}
    for i in range(warmup + runs):
        for name, obj in (("loaded", v), ("prover", sn)):
            ms, rc = timed(lambda: obj.verify(proofs[i % K_BATCH]))
            assert rc == 0
            msb, codes = timed(lambda: obj.verify_batch(proofs))
            assert codes == [0] * K_BATCH
            if i >= warmup:
                t[("verify", name)].append(ms)
                t[("batch", name)].append(msb)
    lines += [f"verify and verify_batch(K = {K_BATCH}) on the loaded key against the prover's key (the same code; alternating, {runs} repetitions), ms:", "",
              "| call | loaded key | prover's key |", "|---|---|---|", f"| verify | {fmt(t[('verify', 'loaded')])} | {fmt(t[('verify', 'prover')])} |",
              f"| verify_batch, K = {K_BATCH} | {fmt(t[('batch', 'loaded')])} | {fmt(t[('batch', 'prover')])} |", ""]
    for what in ("verify", "batch"):
        a, b = t[(what, "loaded")], t[(what, "prover")]
        level = min(a) <= max(b) and min(b) <= max(a)
        lines.append(f"{what}: the ranges {'overlap: level within the spread of the run' if level else 'do NOT overlap'}.")
    lines.append("")
    v.close()
    sn.close()
    return statistics.median(load[True][k]["total"] for k in range(runs)), min(s["total"] for s in load[False]), statistics.median(setup_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verifier_key.md"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bench", action="append", default=[], metavar="LABEL=PATH", help="a bench.py JSON line to list (in the order given)")
    ap.add_argument("--resources", default=None, help="text file with the compiler's resource lines of the new kernels, appended as given")
    a = ap.parse_args()
    assert a.runs >= 10, "at least 10 loads"
    ctx = hip.Context(0)
    lines = ["# A verifier key loaded from its bytes, on the MI355X", "",
             "Written by tools/verifier_key_timing.py: one process, host clock around calls that return synchronised, HIP events for the stages of the device decode.", ""]
    dev_med, host_min, setup_med = one_key(ctx, 2048, a.runs, a.warmup, lines)
    one_key(ctx, 64, a.runs, a.warmup, lines)
    ctx.close()
    wins = dev_med < host_min
    const = hip.wire_decode_constants()
    lines += ["## The default decode", "",
              f"Config-2 key: ss_verifier_from_bytes with the device decode, median {dev_med:.3f} ms; with the host decode, minimum {host_min:.3f} ms; setup, median {setup_med:.3f} ms. "
              + ("The device form's median lies below the host form's minimum: the device decode is the default." if wins else
                 "The device form's median does NOT lie below the host form's minimum: it was measured and did not win; the host decode is the default and the device form "
                 "stays reachable by flag.") + f" The library's default in this run: {'device' if const['device_default'] else 'host'}.", ""]
    if a.bench:
        lines += ["## prove is unchanged: `python bench.py --gpus 1 --steps 20 --warmup 3`, this commit and its parent alternating", "", "| run | value | unit | per step, ms |", "|---|---|---|---|"]
        for item in a.bench:
            label, path = item.split("=", 1)
            row = None
            with open(path) as f:
                for ln in f:
                    ln = ln.strip()
                    if ln.startswith("{") and '"value"' in ln:
                        row = json.loads(ln)
            assert row is not None, f"no JSON line in {path}"
            ms = row.get("ms_per_step", row.get("step_ms", row.get("prove_ms")))
            lines.append(f"| {label} | {row['value']:.4g} | {row.get('unit', '')} | {'' if ms is None else format(ms, '.4f')} |")
        lines.append("")
    if a.resources:
        with open(a.resources) as f:
            lines += ["## The compiler's resource report of the decode kernels (gfx950)", "", f.read().rstrip(), ""]
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
