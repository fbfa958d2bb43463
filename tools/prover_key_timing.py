"""What loading a prover key from its bytes costs, timed on the device's host: the config-2 key (sha256_circuit(bytes(2048)): 2^20 constraints) and the
64-byte key (2^16). One process per run of this tool. Per key: SpartanSNARK(ctx, inst) - setup - as the reference point; SpartanProver.from_bytes with the
device form of the full shape (SP_SHAPE_WIRE_FULL_DEVICE) and with the host form (SP_SHAPE_WIRE_FULL), alternating call by call: the whole call and its
stages (host clock inside the driver; HIP events inside the shape's device decode and its full part); the load with and without trust_digest; the shape
alone, hip.Shape.from_wire with full_device=True against full=True (the host decode is the yardstick); the device memory a loaded key and setup's key
hold; prep_prove_sha256 and prove on the loaded key against setup's key, alternating. Median and min .. max of `runs` repetitions after `warmup`. The
decision between the two forms is stated from the config-2 figures: the device form is the default only if its median lies below the host form's
minimum. --bench takes JSON lines of `python bench.py --gpus 1 --steps 20 --warmup 3` runs (label=path, repeated) for the prove-is-unchanged table.
usage: python tools/prover_key_timing.py [--out profiles/prover_key.md] [--runs 10] [--warmup 2] [--bench this1=a.json --bench parent1=b.json ...]"""
import argparse
import json
import os
import statistics
import struct
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spartan2_amd import frontend, hip, host  # noqa: E402

FORMS = (("device", True), ("host", False))


def fmt(xs, unit=""):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f}){unit}"


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def free_bytes(ctx):
    ctx.synchronize()
    return torch.cuda.mem_get_info()[0]


def shape_offset(key):
    o = 0
    for _ in range(2):
        o += 16 + 64 * struct.unpack_from("<Q", key, o + 8)[0] + 96
    return o


def one_key(ctx, msg_len, runs, warmup, lines):
    inst = frontend.sha256_circuit(bytes(msg_len))
    setup_ms = []
    sn = None
    for _ in range(3):
        if sn is not None:
            sn.close()
        ms, sn = timed(lambda: host.SpartanSNARK(ctx, inst))
        setup_ms.append(ms)
    pkb = sn.pk_to_bytes()
    nnz = sum(sn.shape_info["nnz"])
    lines += [f"## {msg_len}-byte messages: {sn.dims['num_cons']} constraints, {nnz} entries in A, B, C", "",
              f"Key: {len(pkb)} bytes ({len(pkb) / 2**20:.1f} MiB). `SpartanSNARK(ctx, inst)` (setup, 3 calls; the circuit synthesis is not in it): {fmt(setup_ms, ' ms')}.", ""]
    total, load, dec, full = ({True: [], False: []} for _ in range(4))
    for i in range(warmup + runs):
        for _, device in FORMS:
            ms, p = timed(lambda: host.SpartanProver.from_bytes(ctx, pkb, full_device=device, timed=True))
            assert p.vk_digest.tobytes() == sn.vk_digest.tobytes() and p.load_stages["full_device"] == float(device) and p.shape_info == sn.shape_info
            if i >= warmup:
                total[device].append(ms)
                load[device].append(p.load_stages)
                dec[device].append(p.stages)
                full[device].append(p.full_stages)
            p.close()
    lines += [f"`SpartanProver.from_bytes`, the two forms of the full shape alternating, {runs} loads each after {warmup}; ms, median (min .. max):", "",
              "| stage | device form (FULL_DEVICE) | host form (FULL) |", "|---|---|---|",
              f"| whole call (host clock, Python included) | {fmt(total[True])} | {fmt(total[False])} |"]
    for key, label in (("total", "ss_prover_from_bytes"), ("hyrax_keys", "the two Hyrax keys read (2049 + 2 on-curve checks)"), ("shape", "sp_shape_from_wire"),
                       ("ck_create", "the two sp_ck_create"), ("digest", "digest (SHA-256 over the bytes, helper thread)"), ("digest_wait", "wait for the digest behind the rest")):
        lines.append(f"| {label} | {fmt([s[key] for s in load[True]])} | {fmt([s[key] for s in load[False]])} |")
    for key, label in (("parse", "sp_shape_from_wire: parse + checks (host, O(rows))"), ("decode", "sp_shape_from_wire: decode (rows and the full part)")):
        lines.append(f"| {label} | {fmt([s[key] for s in dec[True]])} | {fmt([s[key] for s in dec[False]])} |")
    for key, label in (("upload", "row decode: upload of the raw bytes"), ("entries", "row decode: k_wire_entries"), ("counts_scan", "row decode: k_wire_row_counts + scan"),
                       ("scatter", "row decode: totals read back, allocations, k_wire_scatter")):
        lines.append(f"| {label} (HIP events) | {fmt([s[key] for s in dec[True]])} | - |")
    for key, label in (("filtered", "full part: filtered[] (k_full_filt_counts, scan, k_full_filt_scatter; HIP events)"),
                       ("column_counts", "full part: k_full_col_counts and the read-back of the six counters a column (HIP events)"),
                       ("order", "full part: the walk order on the host (O(columns); host clock)"),
                       ("sort", "full part: uploads of the order, k_full_sort_hist / scan / k_full_sort_scatter per digit (HIP events)"),
                       ("columns", "full part: k_full_col_place, scan, k_full_col_scatter (HIP events)"), ("full_total", "full part: as a whole (host clock)"),
                       ("sort_passes", "full part: digit passes of the sort")):
        lines.append(f"| {label} | {fmt([s[key] for s in full[True]])} | - |")
    lines.append("")
    # with and without the digest pass
    trust = {False: [], True: []}
    for i in range(warmup + runs):
        for t in (False, True):
            ms, p = timed(lambda: host.SpartanProver.from_bytes(ctx, pkb, trust_digest=t))
            if i >= warmup:
                trust[t].append(p.load_stages["total"])
            p.close()
    lines += [f"ss_prover_from_bytes in the default form, digest hashed and compared: {fmt(trust[False], ' ms')}; with `trust_digest` (the stored digest taken as it is): "
              f"{fmt(trust[True], ' ms')}.", ""]
    # the shape alone
    blob = pkb[shape_offset(pkb):-32]
    alone = {True: [], False: []}
    for i in range(warmup + runs):
        for _, device in FORMS:
            s = hip.Shape.from_wire(ctx, blob, full_device=device, full=not device)
            if i >= warmup:
                alone[device].append(s.stages["total"])
            del s
    lines += [f"`sp_shape_from_wire` alone on the shape's {len(blob)} bytes, whole call, ms: SP_SHAPE_WIRE_FULL_DEVICE {fmt(alone[True])}; SP_SHAPE_WIRE_FULL (the host decode "
              f"and sp_shape_from_csr: the yardstick) {fmt(alone[False])}.", ""]
    # device memory
    sn.close()
    base = free_bytes(ctx)
    p = host.SpartanProver.from_bytes(ctx, pkb)
    held_l = base - free_bytes(ctx)
    p.close()
    base = free_bytes(ctx)
    sn = host.SpartanSNARK(ctx, inst)
    held_p = base - free_bytes(ctx)
    lines += [f"Device memory (free memory before and after, this process): the loaded key holds {held_l / 2**20:.1f} MiB, setup's key {held_p / 2**20:.1f} MiB.", ""]
    # proving on both keys
    p = host.SpartanProver.from_bytes(ctx, pkb)
    rng = np.random.default_rng(7)
    tape = np.random.default_rng(1).integers(0, 256, size=(8192, 64), dtype=np.uint8)
    t = {(what, name): [] for what in ("prep", "prove") for name in ("loaded", "setup")}
    for i in range(warmup + runs):
        msg = rng.bytes(msg_len)
        words = {}
        for name, obj in (("loaded", p), ("setup", sn)):
            ms_prep, used = timed(lambda: obj.prep_prove_sha256(msg, tape))
            ms_prove, out = timed(lambda: obj.prove(tape[used:]))
            words[name] = out[0]
            if i >= warmup:
                t[("prep", name)].append(ms_prep)
                t[("prove", name)].append(ms_prove)
        assert (words["loaded"] == words["setup"]).all() and sn.verify(words["loaded"]) == 0
    lines += [f"prep_prove_sha256 and prove on the loaded key against setup's key (the same code and, by sp_shape_compare, the same arrays; alternating, {runs} repetitions), ms:",
              "", "| call | loaded key | setup's key |", "|---|---|---|", f"| prep_prove_sha256 | {fmt(t[('prep', 'loaded')])} | {fmt(t[('prep', 'setup')])} |",
              f"| prove | {fmt(t[('prove', 'loaded')])} | {fmt(t[('prove', 'setup')])} |", ""]
    for what in ("prep", "prove"):
        a, b = t[(what, "loaded")], t[(what, "setup")]
        level = min(a) <= max(b) and min(b) <= max(a)
        lines.append(f"{what}: the ranges {'overlap: level within the spread of the run' if level else 'do NOT overlap'}.")
    lines.append("")
    p.close()
    sn.close()
    return statistics.median(s["total"] for s in load[True]), min(s["total"] for s in load[False]), statistics.median(setup_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prover_key.md"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bench", action="append", default=[], metavar="LABEL=PATH", help="a bench.py JSON line to list (in the order given)")
    ap.add_argument("--resources", default=None, help="text file with the compiler's resource table of the new kernels, appended as given")
    a = ap.parse_args()
    ctx = hip.Context(0)
    lines = ["# A prover key loaded from its bytes, on the MI355X", "",
             "Written by tools/prover_key_timing.py: one process, host clock around calls that return synchronised, HIP events for the stages of the device decode.", ""]
    dev_med, host_min, setup_med = one_key(ctx, 2048, a.runs, a.warmup, lines)
    one_key(ctx, 64, a.runs, a.warmup, lines)
    ctx.close()
    wins = dev_med < host_min
    default = bool(host.lib().ss_prover_full_device_default())
    lines += ["## The default form", "",
              f"Config-2 key: ss_prover_from_bytes with the device form, median {dev_med:.3f} ms; with the host form, minimum {host_min:.3f} ms; setup, median {setup_med:.3f} ms. "
              + ("The device form's median lies below the host form's minimum: the device form is the default of a prover load." if wins else
                 "The device form's median does NOT lie below the host form's minimum: it was measured and did not win; the host form is the default and the device form "
                 "stays reachable by flag.") + f" The library's default in this run: {'device' if default else 'host'}.", ""]
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
            lines += ["## The compiler's resource report of the new kernels (gfx950)", "", f.read().rstrip(), ""]
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
