#!/usr/bin/env python3
"""Is the device code of two source trees the same, kernel by kernel?  (For refactors of host code that sits in a file with
kernels: nothing needs a GPU.)

  compare_device_code.py list  TREE OUTDIR     # device listings of TREE's kernel sources into OUTDIR (build.FLAGS of TREE)
  compare_device_code.py diff  DIR_A DIR_B     # compare two such directories; exit status 1 if a kernel of A is missing from B
                                               # or differs there (kernels only B has are listed, not counted)
  compare_device_code.py stats DIR_A DIR_B     # a markdown table of the kernels whose bodies differ: instructions, vector
                                               # instructions, registers, private segment, LDS, occupancy (A -> B), and the
                                               # kernels that break a bound (exit status 1): private segment 0, LDS and occupancy
                                               # equal, vector instructions <= A + 4, instructions <= A + 2 %

A listing is `hipcc <build.FLAGS minus -fPIC> <the source's extra flags> -S --cuda-device-only`, with the per-compilation
`__hip_cuid_<hex>` replaced by a constant.  Whole files are compared first.  Where they differ the kernels are compared one
by one: the set of `.amdhsa_kernel` names, and for every name the text from its label to `.end_amdhsa_kernel` with the
function ordinal of local labels (`.LBB<n>_`, `.Lfunc_begin<n>`, `.Lfunc_end<n>`, `.Ltmp<n>`; `BB<n>_` in loop comments) masked -- the ordinal follows
the ORDER in which templates are instantiated, which host code decides.  Nothing else is masked, except the run of blanks
between such a label and the comment the compiler pads to a fixed column behind it (its length follows the ordinal's digits).
"""
import importlib.util
import os
import re
import subprocess
import sys

SOURCES = ("csrc/ea_kernels.hip", "csrc/ea_kernels_var.hip", "csrc/ea_capi.hip", "csrc/ea_preprocess.hip")
_ORDINAL = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|Ltmp)\d+|\b(BB)\d+(?=_\d)")  # (BB<n>_<block>: the same label in a loop comment)
_LABEL_PAD = re.compile(r"^(\.LBBN_\d+:)[ \t]+;", re.M)  # the comment behind a label is padded to a column: by the ordinal's digits


def make_listings(tree, outdir):
    pkg = os.path.join(os.path.abspath(tree), "edge_alignment_amd")
    spec = importlib.util.spec_from_file_location("ea_build_of_tree", os.path.join(pkg, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    extra = dict(build.SOURCES)
    os.makedirs(outdir, exist_ok=True)
    procs = []
    for src in SOURCES:
        out = os.path.join(outdir, os.path.basename(src) + ".s")
        cmd = ([build._hipcc()] + [f for f in build.FLAGS if f != "-fPIC"] + list(extra[src]) +
               ["-S", "--cuda-device-only", "-o", out, os.path.join(pkg, src)])
        procs.append((out, cmd, subprocess.Popen(cmd, cwd=pkg)))
    for out, cmd, pr in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
        with open(out) as f:
            text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", f.read())
        with open(out, "w") as f:
            f.write(text)


def kernels(text):
    """name -> text of the kernel from `name:` to `.end_amdhsa_kernel`, local-label ordinals masked"""
    lines = text.split("\n")
    start = {}
    for i, ln in enumerate(lines):
        if ln[:1] not in (".", " ", "\t", "") and ":" in ln:  # `name: ; @name`
            start.setdefault(ln.split(":")[0], i)
    out = {}
    for i, ln in enumerate(lines):
        s = ln.strip()
        if not s.startswith(".amdhsa_kernel "):
            continue
        name = s.split()[1]
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        body = _ORDINAL.sub(lambda m: "." + m.group(1) + "N" if m.group(1) else "BBN", "\n".join(lines[start[name]:end + 1]))
        out[name] = _LABEL_PAD.sub(r"\1 ;", body)
    return out


def diff(dir_a, dir_b):
    bad = 0
    print("| source | lines (A) | kernels A / B | parent against head |")
    print("|---|---|---|---|")
    for src in SOURCES:
        name = os.path.basename(src) + ".s"
        with open(os.path.join(dir_a, name)) as f:
            a = f.read()
        with open(os.path.join(dir_b, name)) as f:
            b = f.read()
        ka, kb = kernels(a), kernels(b)
        if a == b:
            verdict = "byte-identical file"
        else:
            lost, added = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
            differ = sorted(n for n in set(ka) & set(kb) if ka[n] != kb[n])
            if lost or differ:
                bad += 1
                verdict = "DIFFERENT: %d lost, %d added, %d bodies differ" % (len(lost), len(added), len(differ))
                for n in (lost + added + differ)[:20]:
                    print("  !", n, file=sys.stderr)
            elif added:  # new kernels beside the old ones: every kernel of A is in B with the same body
                verdict = "%d kernels added; the %d of A: same names, every body identical after masking label ordinals" % (len(added), len(ka))
                for n in added:
                    print("  +", n, file=sys.stderr)
            else:
                verdict = "same names, every body identical after masking label ordinals (%d kernels)" % len(ka)
        print("| `%s` | %d | %d / %d | %s |" % (os.path.basename(src), a.count("\n"), len(ka), len(kb), verdict))
    return 1 if bad else 0


_INSN = re.compile(r"^\t(v_|s_|ds_|global_|buffer_|flat_|scratch_)\w+", re.M)
_FIELDS = (("VGPR", r"\.amdhsa_next_free_vgpr (\d+)"), ("SGPR", r"\.amdhsa_next_free_sgpr (\d+)"),
           ("private", r"\.amdhsa_private_segment_fixed_size (\d+)"), ("LDS", r"\.amdhsa_group_segment_fixed_size (\d+)"),
           ("occupancy", r"; Occupancy: (\d+)"))  # (the compiler's comment block behind the kernel)
_OCC = re.compile(r"^\s*\.amdhsa_kernel (\S+)$.*?^; Occupancy: (\d+)$", re.M | re.S)


def kernel_stats(body):
    insns = [m.group(0) for m in _INSN.finditer(body)]
    st = {"insns": len(insns), "vector": sum(1 for i in insns if i.startswith("\tv_"))}
    for key, pat in _FIELDS[:-1]:
        st[key] = int(re.search(pat, body).group(1))
    return st


def short_name(name):
    """`_ZN2ea20ea_eval_fused_kernelIdLi1E...EEEvPKv...` -> `ea_eval_fused_kernel<d,1,0,256,1,0,0>`"""
    m = re.match(r"_ZN2ea\d+(\w+?)I((?:[df]|Li\d+E|Lb[01]E)+)EEv", name)
    if not m:
        return name
    return "%s<%s>" % (m.group(1), ",".join(a.strip("LibE") or a for a in re.findall(r"[df]|Li\d+E|Lb[01]E", m.group(2))))


def stats(dir_a, dir_b):
    bad = 0
    keys = ["insns", "vector"] + [k for k, _ in _FIELDS]
    for src in SOURCES:
        name = os.path.basename(src) + ".s"
        with open(os.path.join(dir_a, name)) as f:
            ta = f.read()
        with open(os.path.join(dir_b, name)) as f:
            tb = f.read()
        ka, kb, oa, ob = kernels(ta), kernels(tb), dict(_OCC.findall(ta)), dict(_OCC.findall(tb))
        differ = sorted(n for n in set(ka) & set(kb) if ka[n] != kb[n])
        print("\n`%s`: %d kernels, %d bodies identical after label masking, %d differ\n" % (os.path.basename(src), len(ka), len(ka) - len(differ), len(differ)))
        if not differ:
            continue
        print("| kernel | " + " | ".join(keys) + " | |")
        print("|---|" + "---|" * (len(keys) + 1))
        for n in differ:
            a, b = kernel_stats(ka[n]), kernel_stats(kb[n])
            a["occupancy"], b["occupancy"] = int(oa[n]), int(ob[n])
            broken = [k for k in ("LDS", "occupancy") if a[k] != b[k]]
            broken += ["private"] if b["private"] else []
            broken += ["vector"] if b["vector"] > a["vector"] + 4 else []
            broken += ["insns"] if b["insns"] > a["insns"] * 1.02 else []
            bad += 1 if broken else 0
            print("| `%s` | " % short_name(n) + " | ".join(str(a[k]) if a[k] == b[k] else "%d -> %d" % (a[k], b[k]) for k in keys) +
                  " | %s |" % ("BREAKS " + ", ".join(broken) if broken else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "stats":
        sys.exit(stats(sys.argv[2], sys.argv[3]))
    elif len(sys.argv) == 4 and sys.argv[1] == "list":
        make_listings(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
