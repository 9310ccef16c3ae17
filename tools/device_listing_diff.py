#!/usr/bin/env python3
"""Dev tool: do two trees compile the same device code?  Needs hipcc, no GPU.

  python tools/device_listing_diff.py TREE_A TREE_B qa_sim.hip qa_sim_selfcol.hip ... [--rename OLD=NEW ...] [--rename-re PATTERN=REPL ...] [--jobs N]

Each source (a name under quadrupedal_agility_amd/csrc) is compiled in both trees with the flags HIP_SOURCES (__graft_entry__.py of the tree
this tool lives in) gives it, plus -S --cuda-device-only, and the two listings are compared kernel symbol by kernel symbol: from the kernel's
label to its .end_amdhsa_kernel, i.e. the instructions and the kernel descriptor.  Before the comparison the `;` comments go, local labels
(.L...) are numbered by first appearance inside the kernel (their numbers depend on the kernel's position in the file, their structure does
not), the __hip_cuid_* symbol loses its hash, and --rename OLD=NEW rewrites a symbol of TREE_A that TREE_B names differently (--rename-re: a
regular expression and its replacement, for a template's whole family of mangled names).  The order of
the kernels in a file is not compared.  Prints the symbols only one tree has, the symbols whose text differs, and the totals; exit status 1
if there is any of either."""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g      # noqa: E402

BASE = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]       # compile_library's
LOCAL = re.compile(r"\.L[A-Za-z0-9_$.]+")


def listing(tree, src, out):
    path = os.path.join(tree, "quadrupedal_agility_amd", "csrc", src)
    subprocess.check_call([g._hipcc()] + BASE + dict(g.HIP_SOURCES)[src] + ["-S", "--cuda-device-only", path, "-o", out])
    return open(out).read()


def kernels(text, renames):
    """{kernel symbol: normalised lines from its label to .end_amdhsa_kernel}"""
    for old, new in renames:
        text = old.sub(new, text) if hasattr(old, "sub") else re.sub(r"\b%s\b" % re.escape(old), new, text)
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", text)
    lines = text.split("\n")
    label = {m.group(1): i for i, m in ((i, re.match(r"([A-Za-z_$][\w$.]*):", ln)) for i, ln in enumerate(lines)) if m}
    out = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        name = m.group(1)
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        seen = {}
        body = []
        for raw in lines[label[name]:end + 1]:
            s = raw.split(";", 1)[0].strip()
            if s:
                body.append(LOCAL.sub(lambda t: seen.setdefault(t.group(0), ".L%d" % len(seen)), s))
        out[name] = body
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree_a"); ap.add_argument("tree_b"); ap.add_argument("sources", nargs="+")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="a symbol of TREE_A that TREE_B names NEW")
    ap.add_argument("--rename-re", action="append", default=[], metavar="PATTERN=REPL",
                    help="the same for a family of symbols: a regular expression over TREE_A's listing and its replacement (a template gained a parameter)")
    ap.add_argument("--jobs", type=int, default=min(6, os.cpu_count() or 1))
    a = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in a.rename] + [(re.compile(p), r) for p, r in (x.split("=", 1) for x in a.rename_re)]
    print(f"A = {a.tree_a}\nB = {a.tree_b}\nflags: {' '.join(BASE)} + HIP_SOURCES' + -S --cuda-device-only")
    for old, new in renames:
        print(f"renamed in A: {getattr(old, 'pattern', old)} -> {new}")
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        jobs = {(t, s): pool.submit(listing, tree, s, os.path.join(tmp, f"{t}_{s}.s"))
                for s in a.sources for t, tree in (("a", a.tree_a), ("b", a.tree_b))}
        for s in a.sources:
            ka, kb = kernels(jobs["a", s].result(), renames), kernels(jobs["b", s].result(), [])
            only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
            differ = sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
            print(f"\n{s}: {len(ka)} kernels in A, {len(kb)} in B, {sum(len(v) for v in kb.values())} lines compared")
            for title, names in (("only in A", only_a), ("only in B", only_b), ("text differs", differ)):
                print(f"  {title}: {len(names)}")
                for k in names:
                    print(f"    {k}")
            bad += len(only_a) + len(only_b) + len(differ)
    print(f"\ntotal: {bad} kernel symbols missing or differing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
