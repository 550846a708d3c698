"""The mutant table (tests/mutants.py) against the tree, the built libraries and DESIGN.md.  No GPU.

A stale or missing mutant library is a failure here, not a skip: tests/test_gpu_mutants.py is only worth its name if every library it
loads was built from the table and the sources as they are (tools/build_mutants.py; __graft_entry__.build() runs it)."""
import importlib.util
import json
import os
import re
import subprocess
import sys

import mutants

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "resnet_amd", "csrc")

# killers come from the operator files and the small items of the ragged file; never a batch-256 case, a past-2-GiB case or a test that
# starts child processes of its own
ALLOWED_FILES = {"tests/test_gpu_ops.py", "tests/test_gpu_bf16.py", "tests/test_gpu_ragged.py", "tests/test_gpu_optim.py", "tests/test_gpu_loss_head.py",
                 "tests/test_gpu_eval.py", "tests/test_gpu_dp.py", "tests/test_gpu_input_u8.py", "tests/test_gpu_input_rrc.py", "tests/test_gpu_mix.py",
                 "tests/test_gpu_ema.py", "tests/test_gpu_accum.py", "tests/test_gpu_input_aa.py"}
SPAWNING = ("test_conv_parity_on_the_other_kernel_routes", "test_training_step_bf16_on_the_other_kernel_routes", "test_two_ranks_over_rccl",
            "test_bench_", "test_rccl_one_rank")


def _builder():
    spec = importlib.util.spec_from_file_location("build_mutants", os.path.join(ROOT, "tools", "build_mutants.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_entries_are_well_formed():
    names = [m["name"] for m in mutants.MUTANTS]
    assert len(names) == len(set(names)), "names are not unique"
    assert len(names) >= 130
    for m in mutants.MUTANTS:
        assert re.fullmatch(r"[a-z0-9_]+", m["name"]), m["name"]
        assert m["what"] and m["branch"], m["name"]
        assert m["old"] != m["new"], m["name"]
        assert "asm" not in m["old"] and "asm" not in m["new"], "%s: no inline assembly in a mutant" % m["name"]
        assert m["file"] != "runtime.hip", "%s: no mutant in runtime.hip" % m["name"]
        with open(os.path.join(CSRC, m["file"])) as f:
            n = f.read().count(m["old"])
        assert n == 1, "%s: `old` occurs %d times in %s" % (m["name"], n, m["file"])
        assert 1 <= len(m["killers"]) <= 3, m["name"]
        for k in m["killers"]:
            assert k.split("::")[0] in ALLOWED_FILES, "%s: %s" % (m["name"], k)
            assert not any(s in k for s in SPAWNING), "%s: %s starts processes of its own" % (m["name"], k)
            assert "r50_N33" not in k, "%s: r50_N8 already plans every split and sliced tail the table needs" % m["name"]


def test_every_kernel_file_has_two_mutants_and_the_headers_one_at_most():
    per = {}
    for m in mutants.MUTANTS:
        per[m["file"]] = per.get(m["file"], 0) + 1
    hips = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip") and f != "runtime.hip")
    assert hips == sorted(mutants.KERNEL_FILES)
    for f in hips:
        assert per.get(f, 0) >= 2, "%s has %d mutants" % (f, per.get(f, 0))
    assert sum(n for f, n in per.items() if not f.endswith(".hip")) <= 1, "at most one header mutant (it recompiles every file)"
    assert set(per) <= set(hips) | {"mi_common.hpp"}


def test_no_source_file_carries_a_mutation_hook():
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".hpp", ".h", ".c")):
            with open(os.path.join(CSRC, f), errors="replace") as fh:
                text = fh.read()
            assert not re.search(r"MUTANT|MUTATION", text), f


def test_manifest_matches_the_table_and_the_tree():
    bm = _builder()
    want = bm.expected_manifest()
    assert os.path.exists(bm.MANIFEST), "variants/mutants/MANIFEST.json is missing: run tools/build_mutants.py (build() does)"
    with open(bm.MANIFEST) as f:
        have = json.load(f)
    stale = sorted(n for n in want if have.get(n) != want[n])
    assert not stale, "stale or unbuilt mutant libraries (run tools/build_mutants.py): %s" % stale
    assert sorted(have) == sorted(want), "the manifest names libraries the table lacks: %s" % sorted(set(have) - set(want))
    missing = [n for n in want if not os.path.exists(bm.lib_path(n))]
    assert not missing, "libraries missing: %s" % missing


def test_every_killer_is_collected():
    files = sorted({k.split("::")[0] for k in mutants.all_killers()})
    r = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + files, cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    collected = set(r.stdout.split("\n"))
    missing = [k for k in mutants.all_killers() if k not in collected]
    assert not missing, "killers pytest does not collect: %s" % missing


def test_every_entry_is_in_the_kill_matrix():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    start = text.index("## Suite sensitivity")
    end = text.find("\n## ", start + 5)
    section = text[start:end if end > 0 else len(text)]
    rows = set(re.findall(r"^\| `([a-z0-9_]+)` \|", section, re.M))
    names = {m["name"] for m in mutants.MUTANTS}
    assert names - rows == set(), "not in DESIGN.md's kill matrix: %s" % sorted(names - rows)
    assert rows - names == set(), "in the kill matrix, not in the table: %s" % sorted(rows - names)
