"""Same-instructions check of the world code objects: compiles every moby_amd/csrc/mh_world_*.hip of two source trees to gfx950 assembly with the
Makefile's HIPFLAGS (+ --cuda-device-only -S) and reports, per object and per function, identical or different with both code lengths.  No GPU needed.
usage: python tools/world_asm_diff.py OLD_TREE NEW_TREE [--out DIR] [--jobs N] [--glob PATTERN]     (e.g. OLD_TREE from `git worktree add` or `git archive` of the parent)
--glob picks other code objects of moby_amd/csrc by file name (default mh_world_*.hip; 'mh_artic*.hip' for the articulated stepper's).
--out keeps the .s files (DIR/old, DIR/new; an existing .s is reused, so delete it after editing its tree).  Exit status 1 if any object differs."""
import argparse, concurrent.futures, glob, os, re, subprocess, sys, tempfile

def flags(tree):
    mk = open(os.path.join(tree, "moby_amd", "csrc", "Makefile")).read()
    return re.search(r"^HIPFLAGS \?= (.*)$", mk, re.M).group(1).split(), re.search(r"^HIPCC \?= (.*)$", mk, re.M).group(1)

def assemble(tree, out, pattern):
    os.makedirs(out, exist_ok=True)
    fl, hipcc = flags(tree)
    src = sorted(glob.glob(os.path.join(tree, "moby_amd", "csrc", pattern)))
    return [(s, os.path.join(out, os.path.basename(s)[:-4] + ".s"), [hipcc] + fl + ["--cuda-device-only", "-S"]) for s in src]

def functions(path):
    """{name: (text, codeLenInByte)}; the variant namespace is stripped from names, __hip_cuid_* lines (a hash of the source) are dropped"""
    out, name, body = {}, "(globals)", []
    for ln in open(path):
        if "__hip_cuid_" in ln:
            continue
        m = re.match(r"^(\w+):\s+; @", ln)
        if m:
            out[name] = ("".join(body), None); name, body = m.group(1), []
        body.append(ln)
        m = re.match(r"^; codeLenInByte = (\d+)", ln)
        if m:
            out[name] = ("".join(body), int(m.group(1))); name, body = name + " (tail)", []
    out[name] = ("".join(body), None)
    return out

ap = argparse.ArgumentParser()
ap.add_argument("old"); ap.add_argument("new"); ap.add_argument("--out"); ap.add_argument("--jobs", type=int, default=8)
ap.add_argument("--glob", default="mh_world_*.hip")
a = ap.parse_args()
out = a.out or tempfile.mkdtemp(prefix="world_asm_")
jobs = assemble(a.old, os.path.join(out, "old"), a.glob) + assemble(a.new, os.path.join(out, "new"), a.glob)
with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
    list(ex.map(lambda j: os.path.exists(j[1]) or subprocess.check_call(j[2] + ["-o", j[1], j[0]], cwd=os.path.dirname(j[0])), jobs))
bad = 0
for o in sorted(os.listdir(os.path.join(out, "new"))):
    po = os.path.join(out, "old", o)
    if not os.path.exists(po):
        print("%-30s only in NEW" % o[:-2]); bad += 1; continue
    fo, fn = functions(po), functions(os.path.join(out, "new", o))
    diff = [k for k in sorted(set(fo) | set(fn)) if fo.get(k, ("",))[0] != fn.get(k, ("",))[0]]
    print("%-30s %s" % (o[:-2], "identical (%d functions)" % sum(v[1] is not None for v in fn.values()) if not diff else "DIFFERENT"))
    for k in diff:
        print("    %-60s codeLenInByte %s -> %s" % (k, fo.get(k, (0, "-"))[1], fn.get(k, (0, "-"))[1]))
    bad += bool(diff)
sys.exit(1 if bad else 0)
