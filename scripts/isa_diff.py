#!/usr/bin/env python3
"""Compare the kernels of gfx950 device assembly files, old against new.

    python scripts/isa_diff.py OLD.s NEW.s [NEW2.s ...]

The inputs come from `hipcc --offload-arch=gfx950 -O3 -std=c++17
--cuda-device-only -S`. For every kernel symbol the tool takes the instruction
text from the symbol's label to its function end and the `.amdhsa_` descriptor
block (VGPR / SGPR / scratch / LDS fields), normalises compiler-local label
names and comments, and reports per kernel: identical, differs (with a unified
diff), only-old or only-new. Kernels are matched by demangled name; DROPPED
lists template arguments that the old file still has and the new ones do not
(the argument is stripped only at the value the surviving kernel was built
with). The comparison is textual: the tool knows no instruction.
"""
import difflib
import re
import subprocess
import sys

# kernel name -> (index of the template argument removed, value it had)
DROPPED = {
    "fmda::gru_fwd_kernel": (5, "false"),
    "fmda::gru_bwd_kernel": (5, "false"),
    "fmda::gru_fwd_v3_kernel": (4, "3"),
    "fmda::gru_bwd_v3_kernel": (4, "7"),
}
LOCAL = re.compile(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b")


def kernels(path):
    """{mangled symbol: (instruction lines, descriptor lines)}"""
    lines = open(path).read().split("\n")
    out = {}
    for sym in (m.group(1) for ln in lines
                if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))):
        start = lines.index(next(ln for ln in lines
                                 if ln.startswith(sym + ":")))
        text, desc, in_desc = [], [], False
        for ln in lines[start + 1:]:
            if re.match(r"\.Lfunc_end\d+:", ln):
                break
            ln = ln.split(";")[0].replace(sym, "<self>").rstrip()
            ln = LOCAL.sub(lambda m: ".L%s%s" % (m.group(1), m.group(2) or ""),
                           ln)
            if ln.strip().startswith(".amdhsa_kernel"):
                in_desc = True
            elif ln.strip() == ".end_amdhsa_kernel":
                in_desc = False
            elif in_desc:
                desc.append(ln.strip())
            elif ln.strip() and not ln.strip().startswith((".section",
                                                           ".p2align")):
                text.append(ln)
        out[sym] = (text, desc)
    return out


def demangle(syms):
    res = subprocess.run(["c++filt"], input="\n".join(syms), text=True,
                         capture_output=True, check=True)
    return dict(zip(syms, res.stdout.split("\n")))


def key(name, strip):
    """Demangled name without return type and parameter list."""
    m = re.match(r"(?:void )?([\w:]+)(?:<([^>]*)>)?", name)
    base, args = m.group(1), (m.group(2) or "").split(", ")
    if strip and base in DROPPED:
        i, val = DROPPED[base]
        if i < len(args) and args[i] == val:
            del args[i]
    return "%s<%s>" % (base, ", ".join(args)) if args != [""] else base


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    old = kernels(argv[1])
    new = {}
    for p in argv[2:]:
        new.update(kernels(p))
    dm = demangle(list(old) + list(new))
    old = {key(dm[s], True): v for s, v in old.items()}
    new = {key(dm[s], False): v for s, v in new.items()}
    counts = {"identical": 0, "differs": 0, "only-old": 0, "only-new": 0}
    for k in sorted(set(old) | set(new)):
        if k not in new:
            state = "only-old"
        elif k not in old:
            state = "only-new"
        else:
            state = "identical" if old[k] == new[k] else "differs"
        counts[state] += 1
        print("%-9s %s" % (state, k))
        if state == "differs":
            for part, name in ((0, "text"), (1, "descriptor")):
                sys.stdout.write("\n".join(difflib.unified_diff(
                    old[k][part], new[k][part], "old " + name, "new " + name,
                    lineterm="")) + "\n")
    print("summary: " + ", ".join("%d %s" % (n, s) for s, n in counts.items()))
    return 1 if counts["differs"] or counts["only-new"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
