"""CPU: tests/switch_registry.py against the product's sources and the test files. A SPARTAN_* switch that is read but not registered, registered but
no longer read, or a path / scheduling value that no test sets fails here - before a GPU run could miss it. Reads the test files as text (no GPU
test module is imported)."""
import ast
import glob
import io
import os
import re
import tokenize

import pytest

import switch_registry as reg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_C_READ = re.compile(r'getenv\(\s*"SPARTAN_([A-Z0-9_]+)"')
_PY_READ = re.compile(r'''(?:environ\.get\(|environ\[|getenv\()\s*["']SPARTAN_([A-Z0-9_]+)["']''')


def _product_files():
    pats = [f"spartan2_amd/**/*.{ext}" for ext in ("hip", "hpp", "cpp", "h", "py")] + ["include/**/*"]
    out = set()
    for p in pats:
        out.update(f for f in glob.glob(os.path.join(ROOT, p), recursive=True) if os.path.isfile(f))
    return sorted(out)


def switches_read(files=None):
    """{name: [file, ...]} of every SPARTAN_* variable read through getenv (C / C++) or os.environ / os.getenv (Python)."""
    found = {}
    for f in files if files is not None else _product_files():
        with open(f, encoding="utf-8", errors="replace") as fh:
            text = fh.read()
        for name in set((_PY_READ if f.endswith(".py") else _C_READ).findall(text)):
            found.setdefault(name, []).append(os.path.relpath(f, ROOT))
    return found


def code_text(path):
    """The file's source with its comments and docstrings blanked out: what sets a switch must be code, not a remark about it."""
    with open(os.path.join(ROOT, path), encoding="utf-8") as fh:
        src = fh.read()
    lines = src.splitlines(keepends=True)
    for tok in tokenize.generate_tokens(io.StringIO(src).readline):
        if tok.type == tokenize.COMMENT:
            (r, c), _ = tok.start, tok.end
            lines[r - 1] = lines[r - 1][:c] + "\n"
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and node.body:
            d = node.body[0]
            if isinstance(d, ast.Expr) and isinstance(d.value, ast.Constant) and isinstance(d.value.value, str):
                for i in range(d.lineno - 1, d.end_lineno):
                    lines[i] = "\n"
    return "".join(lines)


def _functions_of(path):
    with open(os.path.join(ROOT, path), encoding="utf-8") as fh:
        tree = ast.parse(fh.read())
    return {n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))}


_ENV_STRING = re.compile(r"SPARTAN_[A-Z0-9_]+=\S+(?: SPARTAN_[A-Z0-9_]+=\S+)*")


def env_settings(path):
    """{(NAME, value)} of the child-process environments a test file spells out: string constants made only of SPARTAN_X=v words."""
    with open(os.path.join(ROOT, path), encoding="utf-8") as fh:
        tree = ast.parse(fh.read())
    out = set()
    for n in ast.walk(tree):
        if isinstance(n, ast.Constant) and isinstance(n.value, str) and _ENV_STRING.fullmatch(n.value):
            for kv in n.value.split():
                k, v = kv.split("=", 1)
                out.add((k[len("SPARTAN_"):], v))
    return out


def sets_value(code, settings, name, value, sets):
    return sets in code if sets else (name, value) in settings


def uncovered_values(registry=None):
    """["NAME=value: why", ...] for every value of a switch whose covering test does not exist or does not set it."""
    registry = reg.SWITCHES if registry is None else registry
    bad, codes, funcs, settings = [], {}, {}, {}
    for s in registry.values():
        if s.cls == reg.PATH and not s.values:
            bad.append(f"{s.name}: a path switch without a non-default value to test")
        for value, covers in s.values.items():
            if not covers:
                bad.append(f"{s.name}={value}: no test")
            for cv in covers:
                path, _, fn = cv.test.partition("::")
                if not os.path.isfile(os.path.join(ROOT, path)):
                    bad.append(f"{s.name}={value}: {path} does not exist")
                    continue
                if path not in codes:
                    codes[path], funcs[path], settings[path] = code_text(path), _functions_of(path), env_settings(path)
                if fn not in funcs[path]:
                    bad.append(f"{s.name}={value}: {path} has no {fn}")
                elif not sets_value(codes[path], settings[path], s.name, value, cv.sets):
                    bad.append(f"{s.name}={value}: {path} does not set it ({cv.sets or f'SPARTAN_{s.name}={value}'} not found)")
    return bad


def test_every_switch_read_is_registered():
    read = switches_read()
    assert read, "no SPARTAN_* read found: the scan is broken"
    missing = {n: f for n, f in read.items() if n not in reg.SWITCHES}
    assert not missing, f"read but not in tests/switch_registry.py: {missing}"


def test_every_registered_switch_is_still_read():
    read = switches_read()
    stale = sorted(n for n in reg.SWITCHES if n not in read)
    assert not stale, f"registered but no longer read by the product: {stale}"


def test_every_value_has_a_test_that_sets_it():
    bad = uncovered_values()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", sorted(reg.SWITCHES))
def test_registry_entry_is_well_formed(name):
    s = reg.SWITCHES[name]
    assert s.cls in (reg.PATH, reg.SCHEDULING, reg.TRACE)
    assert s.default not in s.values, "the default is not a value to test"
    assert all(isinstance(v, str) and v and " " not in v for v in s.values)
    src = s.source.split(":")[0]
    with open(os.path.join(ROOT, src), encoding="utf-8", errors="replace") as fh:
        assert f"SPARTAN_{name}" in fh.read(), f"{s.source} does not read SPARTAN_{name}"


def test_child_runs_set_only_registered_values():
    """Every SPARTAN_X=v a child run sets is a registered value of a registered switch: a value the parser does not keep, or a typo in a name, would
    run the default path under a test that claims another."""
    bad = []
    for path in ("tests/test_gpu_switched_paths.py", "tests/test_gpu_abi_gaps.py"):
        for name, value in sorted(env_settings(path)):
            s = reg.SWITCHES.get(name)
            if s is None or value not in s.values:
                bad.append(f"{path}: SPARTAN_{name}={value}")
    assert not bad, bad


def test_the_guard_sees_a_new_switch_and_a_missing_value(tmp_path):
    """The checks above fail as they should: a new getenv in a product file is found by name, a registered value whose child-run parameter is gone
    is named."""
    f = tmp_path / "scratch.hip"
    f.write_text('static int x() { const char* e = getenv("SPARTAN_NEW_THING"); return e ? 1 : 0; }\n'
                 'static bool y() { return getenv( "SPARTAN_COMB_BITS") != nullptr; }\n')
    p = tmp_path / "scratch.py"
    p.write_text('import os\nA = os.environ.get("SPARTAN_PY_THING", "0")\nB = os.environ["SPARTAN_PY_OTHER"]\n')
    read = switches_read([str(f), str(p)])
    assert set(read) == {"NEW_THING", "COMB_BITS", "PY_THING", "PY_OTHER"}
    fake = dict(reg.SWITCHES)
    fake["COMB_BITS"] = reg.Switch("COMB_BITS", "13", reg.PATH, {"9": (reg.Cover(reg.SWITCHED),)})
    assert uncovered_values(fake) == ["COMB_BITS=9: tests/test_gpu_switched_paths.py does not set it (SPARTAN_COMB_BITS=9 not found)"]
    # only whole SPARTAN_X=v words of an environment string count: not a longer value, not a mention inside a message
    t = tmp_path / "test_scratch.py"
    t.write_text('P = ["SPARTAN_TAIL_LOG2=15 SPARTAN_ROUND_TRACE=1"]\nM = "no round lines (SPARTAN_TAIL_BUDGET=0)"\n# "SPARTAN_GATE=0"\n')
    assert env_settings(str(t)) == {("TAIL_LOG2", "15"), ("ROUND_TRACE", "1")}
