"""Is the gfx950 assembly of every csrc/*.hip the same as at another revision?  (no GPU needed: hipcc cross-compiles)

    python tools/isa_identical.py <git-rev> [-DNAME[=V] ...] [--only a,b,...] [--keep DIR]

Checks <git-rev>'s autoposeestimation_amd/csrc and include out into a temporary directory, compiles every .hip of that tree and of the
working tree to device assembly (each tree with its own Makefile's FLAGS, plus the -D switches given here; at most 16 jobs), drops the
lines that carry the translation unit's `__hip_cuid_<hash>` symbol and compares the rest as text.  Prints one line per file and, where
the text differs, the symbols whose bodies differ.  Exit status 1 when any file differs.  This is the proof that a change of the shared
device headers left every kernel's instructions, registers and LDS as they were -- and so its speed."""
import argparse, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "autoposeestimation_amd/csrc"


def make_var(tree, name, default=None):
    m = re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, open(os.path.join(tree, CSRC, "Makefile")).read(), re.M)
    return m.group(1).strip() if m else default


def assembly(tree, out, defs, only):
    """-> {file.hip: assembly text without the cuid lines, or None when it does not compile}"""
    os.makedirs(out)
    csrc = os.path.join(tree, CSRC)
    flags = make_var(tree, "FLAGS").replace("$(ARCH)", os.environ.get("ARCH", make_var(tree, "ARCH", "gfx950"))).split()
    hipcc = os.environ.get("HIPCC", make_var(tree, "HIPCC", "hipcc"))
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip") and (not only or f[:-4] in only))

    def one(f):
        s = os.path.join(out, f[:-4] + ".s")
        r = subprocess.run([hipcc] + flags + defs + ["--cuda-device-only", "-S", f, "-o", s], cwd=csrc, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            return f, None
        return f, "".join(ln for ln in open(s) if "__hip_cuid_" not in ln)

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        return dict(ex.map(one, srcs))


def by_symbol(text):
    """the text cut at every global label: {symbol: lines up to the next one}"""
    parts, cur = {"<head>": []}, "<head>"
    for ln in text.splitlines():
        m = re.match(r"([A-Za-z_$][\w$.]*):", ln)
        if m and not m.group(1).startswith(".L"):
            cur = m.group(1)
            parts[cur] = []
        parts[cur].append(ln)
    return parts


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev")
    ap.add_argument("-D", dest="defs", action="append", default=[], metavar="NAME[=V]")
    ap.add_argument("--only", default="", help="comma-separated source names without .hip (e.g. the four ablation sources)")
    ap.add_argument("--keep", default="", help="write the .s files under this directory instead of a temporary one")
    a = ap.parse_args()
    defs = ["-D" + d for d in a.defs]
    only = {s for s in a.only.split(",") if s}
    with tempfile.TemporaryDirectory() as tmp:
        work = a.keep or tmp
        old = os.path.join(tmp, "old_tree")
        os.makedirs(old)
        ar = subprocess.run(["git", "-C", REPO, "archive", a.rev, CSRC, "include"], capture_output=True)
        if ar.returncode != 0:
            sys.exit(ar.stderr.decode())
        subprocess.run(["tar", "-x", "-C", old], input=ar.stdout, check=True)
        was = assembly(old, os.path.join(work, "asm_" + re.sub(r"\W", "_", a.rev)), defs, only)
        now = assembly(REPO, os.path.join(work, "asm_worktree"), defs, only)
    bad = 0
    for f in sorted(set(was) | set(now)):
        if f not in was or f not in now:
            print("%-24s only in %s" % (f, a.rev if f in was else "the working tree"))
            bad += 1
        elif was[f] is None or now[f] is None:
            print("%-24s DOES NOT COMPILE (%s)" % (f, a.rev if was[f] is None else "working tree"))
            bad += 1
        elif was[f] == now[f]:
            print("%-24s identical (%d lines)" % (f, was[f].count("\n")))
        else:
            bad += 1
            p, q = by_symbol(was[f]), by_symbol(now[f])
            names = [s for s in list(p) + [s for s in q if s not in p] if p.get(s) != q.get(s)]
            d = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
            print("%-24s DIFFERS in %d symbol(s):" % (f, len(names)))
            for s in d[:40]:
                print("    " + s[:200])
    print("%d of %d sources identical to %s%s" % (len(set(was) | set(now)) - bad, len(set(was) | set(now)), a.rev, (" with " + " ".join(defs)) if defs else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
