"""The suite measured against planted faults ("Suite sensitivity"; the table is tests/mutants.py).

Every mutant is a second build of the library with ONE value fault (tools/build_mutants.py -> variants/mutants/libresnet_mi_<name>.so).
Its killers -- checks of this suite that reach the mutated branch -- run in a child process with RESNET_MI_LIB pointing at it:

    timeout -k 10 180 python -m pytest -q -x <killer node ids>

* control: one child first runs the union of all killers on the normal library and must exit 0; without it a kill proves nothing.
* per mutant: the child must exit with status 1 AND its report must show a failed assertion (pytest's "E   AssertionError" / "E   assert"
  lines).  Exit 0: the mutant survived -- a hole in the suite; the test fails with the entry's `what`.  Any other status (a signal, 124 /
  137 from the time limit, 134, 139, pytest's 2..5) or a GPU memory fault in the output: the mutant broke the value-only rule or the
  machine is unwell; the test fails and every later test of this module fails at once without starting another process (as
  tests/test_gpu_routes.py stops).  Nothing is retried.

The children run strictly one after another and this process never initialises the GPU: one process has the device open at a time.
The time limits are hang guards, not measurements (180 s per mutant; the control runs every killer: 900 s).
"""
import os
import re
import subprocess
import sys
import time

import pytest

import mutants

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIBS = os.path.join(ROOT, "variants", "mutants")
LIMIT, CONTROL_LIMIT = 180, 900
CASUALTY = []    # the first child that died, timed out or faulted the device
TIMES = {}       # child -> wall seconds
STATE = {}       # "control": True once the control child has passed
ASSERTION = re.compile(r"^E\s+(AssertionError|assert\b)", re.M)


def run_child(what, killers, lib, limit):
    """one child under its own time limit; returns (exit status, output) or fails the test and marks the casualty"""
    if CASUALTY:
        pytest.fail("not started: an earlier child of this module was a casualty (%s)" % CASUALTY[0])
    env = dict(os.environ)
    env.pop("RESNET_MI_LIB", None)
    if lib:
        env["RESNET_MI_LIB"] = lib
    argv = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider"] + list(killers)
    t0 = time.time()
    try:
        r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=limit + 60, cwd=ROOT)
    except subprocess.TimeoutExpired:
        CASUALTY.append("%s: no end after %d s" % (what, limit + 60))
        pytest.fail(CASUALTY[0])
    TIMES[what] = time.time() - t0
    text = r.stdout + r.stderr
    if r.returncode not in (0, 1) or "illegal memory access" in text or "Memory access fault" in text:
        CASUALTY.append("%s: exit status %d\n%s" % (what, r.returncode, text[-3000:]))
        pytest.fail(CASUALTY[0])
    return r.returncode, text


@pytest.fixture(scope="module")
def control():
    """the union of all killers on the normal library: started by the first mutant test, judged by every one"""
    if "control" not in STATE:
        STATE["control"] = None  # a failure here is not repeated
        rc, text = run_child("control", mutants.all_killers(), None, CONTROL_LIMIT)
        assert rc == 0, "the killers do not pass on the normal library:\n%s" % text[-4000:]
        m = re.search(r"(\d+) passed", text)
        assert m and int(m.group(1)) == len(mutants.all_killers()) and " skipped" not in text.splitlines()[-1], text[-1500:]
        STATE["control"] = True
    if not STATE["control"]:
        pytest.fail("the control child failed (see the first test of this module)")
    return True


@pytest.fixture(scope="module", autouse=True)
def _summary():
    t0 = time.time()
    yield
    print("\nmutant children, wall seconds (module %.0f s): " % (time.time() - t0) + ", ".join("%s %.1f" % kv for kv in TIMES.items()))


def test_control_runs_every_killer_on_the_normal_library(control):
    assert control


@pytest.mark.parametrize("name", [m["name"] for m in mutants.MUTANTS])
def test_mutant_is_killed(name, control):
    m = mutants.by_name(name)
    lib = os.path.join(LIBS, "libresnet_mi_%s.so" % name)
    assert os.path.exists(lib), "%s is missing: tools/build_mutants.py builds it (tests/test_mutants_table.py checks that it is fresh)" % lib
    rc, text = run_child(name, m["killers"], lib, LIMIT)
    assert rc != 0, "SURVIVED: %s (%s, %s) -- none of %s noticed" % (m["what"], m["file"], m["branch"], m["killers"])
    assert ASSERTION.search(text) and re.search(r"\b1 failed\b", text), \
        "%s: the child failed without a checker's assertion in its report:\n%s" % (name, text[-3000:])
