#!/usr/bin/env python3
"""Build the mutant libraries of tests/mutants.py ("Suite sensitivity").

Per entry: the patched copy of its one source file goes to variants/mutants/src_<name>/, is compiled with the Makefile's HIPFLAGS (-I the
real csrc, so every other header is the real one; a header mutant's copy lies in front of it on the include path and every .hip file is
recompiled), and linked with the normal build's other objects to variants/mutants/libresnet_mi_<name>.so.  variants/mutants/MANIFEST.json
holds name -> sha256(source file + old + new + flags + every other source and header of the library); a rerun rebuilds only entries whose
hash changed or whose library is missing.  The other sources count because their objects are linked in: a library left from before an
entry point was added lacks it, and the binding refuses to load such a library.
The normal build (make in resnet_amd/csrc) must have run: its objects are linked in.

  python tools/build_mutants.py [-j JOBS] [name ...]        JOBS <= 16 (default 8)
"""
import argparse
import concurrent.futures as cf
import hashlib
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "resnet_amd", "csrc")
OUT = os.path.join(ROOT, "variants", "mutants")
MANIFEST = os.path.join(OUT, "MANIFEST.json")
sys.path.insert(0, os.path.join(ROOT, "tests"))


def makefile_vars():
    """HIPCC, ARCH, HIPFLAGS, HIP_SRCS and C_SRCS as resnet_amd/csrc/Makefile sets them"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        text = f.read()
    v = {}
    for name in ("HIPCC", "ARCH", "HIPFLAGS", "HIP_SRCS", "C_SRCS"):
        m = re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M)
        if not m:
            raise SystemExit("build_mutants: the Makefile sets no %s" % name)
        v[name] = m.group(1).strip()
    v["HIPCC"] = os.environ.get("HIPCC", v["HIPCC"])
    v["HIPFLAGS"] = v["HIPFLAGS"].replace("$(ARCH)", v["ARCH"])
    return v


def patched(m):
    """the mutant's source text; fails loudly unless `old` occurs exactly once"""
    with open(os.path.join(CSRC, m["file"])) as f:
        src = f.read()
    n = src.count(m["old"])
    if n != 1:
        raise SystemExit("build_mutants: %s: `old` occurs %d times in %s (exactly one wanted)" % (m["name"], n, m["file"]))
    if m["old"] == m["new"]:
        raise SystemExit("build_mutants: %s: old == new" % m["name"])
    return src, src.replace(m["old"], m["new"])


def tree_digest():
    """sha256 over everything the library is built from: resnet_amd/csrc (sources, headers, Makefile) and include/"""
    h = hashlib.sha256()
    files = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".c", ".h", ".hpp")) or f == "Makefile"]
    inc = os.path.join(ROOT, "include")
    files += [os.path.join(inc, f) for f in os.listdir(inc) if f.endswith(".h")]
    for path in sorted(files):
        with open(path, "rb") as f:
            h.update(os.path.basename(path).encode() + b"\0" + f.read() + b"\0")
    return h.hexdigest()


def entry_hash(m, src, flags, tree=None):
    h = hashlib.sha256()
    for part in (src, m["old"], m["new"], flags, tree or tree_digest()):
        h.update(part.encode())
        h.update(b"\0")
    return h.hexdigest()


def lib_path(name):
    return os.path.join(OUT, "libresnet_mi_%s.so" % name)


def prepare(m, text, mk):
    """write the patched copy; returns the compile jobs [(source, object)] of the entry"""
    sdir = os.path.join(OUT, "src_" + m["name"])
    os.makedirs(sdir, exist_ok=True)
    with open(os.path.join(sdir, m["file"]), "w") as f:
        f.write(text)
    srcs = [m["file"]]
    if not m["file"].endswith(".hip"):
        # a header mutant: a quoted include looks beside the including file first, so every .hip file is compiled from a copy that lies
        # beside the patched header -- the patched copy then comes before the real one on the include path
        srcs = mk["HIP_SRCS"].split()
        for s in srcs:
            with open(os.path.join(CSRC, s)) as f:
                body = f.read()
            with open(os.path.join(sdir, s), "w") as f:
                f.write(body)
    return [(os.path.join(sdir, s), os.path.join(sdir, os.path.splitext(s)[0] + ".o")) for s in srcs]


def hip_flags(mk):
    """the Makefile's HIPFLAGS with its relative include directories made absolute (the patched copies lie elsewhere)"""
    return [a for a in mk["HIPFLAGS"].split() if a not in ("-I.", "-I../../include")] + ["-I" + CSRC, "-I" + os.path.join(ROOT, "include")]


def compile_one(mk, src, obj):
    t0 = time.time()
    subprocess.check_call([mk["HIPCC"]] + hip_flags(mk) + ["-c", src, "-o", obj])
    return time.time() - t0


def link_one(m, objs, mk):
    """the entry's objects + the normal build's others -> libresnet_mi_<name>.so"""
    mine = {os.path.basename(o): o for o in objs}
    link = []
    for s in mk["HIP_SRCS"].split() + mk["C_SRCS"].split():
        base = os.path.splitext(s)[0] + ".o"
        o = mine.get(base) or os.path.join(CSRC, base)
        if not os.path.exists(o):
            raise SystemExit("build_mutants: %s is missing: run make in resnet_amd/csrc first" % o)
        link.append(o)
    tmp = lib_path(m["name"]) + ".tmp"
    subprocess.check_call([mk["HIPCC"], "--offload-arch=" + mk["ARCH"], "-shared", "-fPIC", "-o", tmp] + link + ["-ldl", "-lm"])
    os.replace(tmp, lib_path(m["name"]))
    for o in objs:
        os.remove(o)


def expected_manifest():
    """name -> hash for the table and the tree as they are (tests/test_mutants_table.py compares the file with this)"""
    import mutants
    mk = makefile_vars()
    tree = tree_digest()
    return {m["name"]: entry_hash(m, patched(m)[0], mk["HIPFLAGS"], tree) for m in mutants.MUTANTS}


def main():
    import mutants
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("names", nargs="*")
    a = ap.parse_args()
    jobs = max(1, min(16, a.j))
    mk = makefile_vars()
    os.makedirs(OUT, exist_ok=True)
    try:
        with open(MANIFEST) as f:
            have = json.load(f)
    except (OSError, ValueError):
        have = {}
    table = [m for m in mutants.MUTANTS if not a.names or m["name"] in a.names]
    names = [m["name"] for m in mutants.MUTANTS]
    if len(set(names)) != len(names):
        raise SystemExit("build_mutants: names are not unique")
    todo = []
    tree = tree_digest()
    for m in table:
        src, text = patched(m)
        h = entry_hash(m, src, mk["HIPFLAGS"], tree)
        if have.get(m["name"]) != h or not os.path.exists(lib_path(m["name"])):
            todo.append((m, text, h))
    # entries that left the table: their libraries go, so that the directory holds what the manifest names
    for name in [n for n in have if n not in names]:
        have.pop(name)
        if os.path.exists(lib_path(name)):
            os.remove(lib_path(name))
    t0 = time.time()
    failed = []

    def save():
        with open(MANIFEST + ".tmp", "w") as f:
            json.dump(have, f, indent=1, sort_keys=True)
        os.replace(MANIFEST + ".tmp", MANIFEST)

    with cf.ThreadPoolExecutor(jobs) as pool:  # one compile per job; an entry is linked when its last object is there
        pending = {}
        futs = {}
        for m, text, h in todo:
            units = prepare(m, text, mk)
            pending[m["name"]] = dict(m=m, h=h, left=len(units), objs=[o for _, o in units], secs=0.0, bad=False)
            for src, obj in units:
                futs[pool.submit(compile_one, mk, src, obj)] = m["name"]
        for fu in cf.as_completed(futs):
            st = pending[futs[fu]]
            st["left"] -= 1
            try:
                st["secs"] += fu.result()
            except subprocess.CalledProcessError as e:
                st["bad"] = True
                failed.append("%s: %s" % (futs[fu], e))
            if st["left"] == 0 and not st["bad"]:
                try:
                    link_one(st["m"], st["objs"], mk)
                    have[futs[fu]] = st["h"]
                    print("built %-34s %5.1f s of compiles" % (futs[fu], st["secs"]), flush=True)
                except (subprocess.CalledProcessError, SystemExit) as e:
                    failed.append("%s: %s" % (futs[fu], e))
                save()
    save()
    size = sum(os.path.getsize(lib_path(n)) for n in have if os.path.exists(lib_path(n)))
    print("mutants: %d in the table, %d built now in %.0f s with %d jobs, %.1f MB of libraries" % (len(names), len(todo) - len(failed), time.time() - t0, jobs, size / 1e6))
    if failed:
        raise SystemExit("build_mutants: FAILED\n" + "\n".join(failed))


if __name__ == "__main__":
    main()
