"""CPU: spartan2_amd/host/proof_layout.hpp - the one statement of the flat proof layouts - against proofs the oracle proves and serialises on the CPU:
word count, wire length, bytes in both directions, the parsed view's pointers and the refusal of malformed bytes (tests/native/layout_check.hip,
host code only, linked against libspartan_hip.so for the wire sink / source)."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from spartan2_amd import frontend, hip, host
from test_oracle_wire import CASES as SPARTAN_CASES

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def layout_check(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    hip.lib()  # the library must have been built
    exe = str(tmp_path_factory.mktemp("layout") / "layout_check")
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-pthread", "-w", "-o", exe, os.path.join(HERE, "native", "layout_check.hip"),
                    "-L" + hip.LIB_DIR, "-lspartan_hip", "-Wl,-rpath," + hip.LIB_DIR], check=True, capture_output=True, timeout=900)
    return exe


def _tape(label, blocks=32768):
    return np.frombuffer(hashlib.shake_256(label).digest(64 * blocks), dtype=np.uint8).reshape(blocks, 64).copy()


def _dims(d):
    return [int(d[k]) for k in host.DIM_NAMES]


def _run(exe, path, kind, dims_step, dims_core, head, words, data):
    head = [kind] + dims_step + dims_core + head + [len(words), len(data)]
    with open(path, "wb") as f:
        f.write(np.asarray(head, dtype=np.uint64).tobytes())
        f.write(np.ascontiguousarray(words, dtype=np.uint64).tobytes())
        f.write(data)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and ": 0 mismatches" in out.stdout, out.stdout + out.stderr


def _synthetic(n, groups, core_groups):
    return [frontend.synthetic_circuit(groups, 0xA5, num_public=1, witness_seed=50 + i) for i in range(n)], frontend.synthetic_circuit(core_groups, 0xA5, num_public=1, witness_seed=7)


def _golden_small():
    return _synthetic(3, 8, 2) + (b"golden-tape-nn", "neutronnova_small.json")


def _core_larger():
    return _synthetic(4, 3, 8) + (b"layout-core-larger", None)


def _golden_rest():
    steps = [frontend.sha256_rest_circuit(bytes([i]) * 32) for i in range(2)]
    return steps, steps[0], b"golden-tape-nn-rest", "neutronnova_rest.json"


def _shared():
    mk = lambda ws: frontend.synthetic_circuit(30, 0x77, num_public=2, shared_permille=300, precommitted_permille=1000, witness_seed=ws)
    return [mk(5), mk(5)], mk(5), b"layout-shared", None


def _other_split():
    """two precommitted rows in a step against one in the core: after equalize the core's rows split 1 | 1 where a step's split 2 | 0"""
    return _synthetic(3, 30, 2) + (b"layout-other-split", None)


NN_CASES = {"golden_small_core_grows": _golden_small, "step_grows": _core_larger, "golden_rest_only": _golden_rest, "shared_commitment": _shared,
            "core_splits_rows_differently": _other_split}


@pytest.mark.parametrize("name", list(NN_CASES))
def test_neutronnova_layout_against_the_oracle(layout_check, tmp_path, name):
    steps, core, tape, gold_file = NN_CASES[name]()
    nn = ol.OracleNeutronNova(steps, core)
    words, _, _ = nn.prove(_tape(tape))
    data = nn.proof_to_bytes(words)
    back = nn.proof_from_bytes(data)
    assert back is not None and (back == words).all()
    gold = [0, 0]
    if gold_file:
        with open(os.path.join(GOLD, gold_file)) as f:
            g = json.load(f)
        assert hashlib.sha256(data).hexdigest() == g["wire_sha256"]
        gold = [g["proof_words"], g["wire_len"]]
    (_, ds), (_, dc) = host.pad_shapes_equalized(steps[0], core)
    if name == "golden_small_core_grows":
        assert dc["num_cons"] > host.pad_shape(core)[1]["num_cons"]  # equalize grew the core
    if name == "step_grows":
        assert ds["num_cons"] > host.pad_shape(steps[0])[1]["num_cons"]
    if name == "core_splits_rows_differently":
        assert (ds["num_precommitted"], ds["num_rest"]) == (4096, 0) and (dc["num_precommitted"], dc["num_rest"]) == (2048, 2048)
    if name == "golden_rest_only":
        assert ds["num_shared"] == 0 and ds["num_precommitted"] == 0
    if name == "shared_commitment":
        assert ds["num_shared_unpadded"] > 0 and data[0] == 1  # Some(comm_W_shared)
    info = nn.info
    head = [len(steps), info["nb"], info["nx"], info["ny"], info["vc_vars"], info["vc_cons"], info["vc_public"]] + gold
    _run(layout_check, tmp_path / "case.bin", 0, _dims(ds), _dims(dc), head, words, data)


@pytest.mark.parametrize("name", list(SPARTAN_CASES))
def test_spartan_layout_against_the_oracle(layout_check, tmp_path, name):
    inst = SPARTAN_CASES[name]()
    sp = ol.OracleSpartan(inst)
    tape = ol.make_tape(3, 8192)
    used = sp.prep_prove(tape)
    words, _, _ = sp.prove(tape[used:])
    data = sp.proof_to_bytes(words)
    _, d = host.pad_shape(inst)
    _run(layout_check, tmp_path / "case.bin", 1, _dims(d), _dims(d), [0] * 9, words, data)
