"""Compare two hipcc -Rpass-analysis=kernel-resource-usage logs kernel by kernel.

    python3 tools/resource_diff.py OLD.txt NEW.txt [--markdown]

A kernel of NEW is matched to the kernel of OLD with the same demangled name,
or -- a template that gained trailing defaulted parameters -- to the one whose
name it becomes once trailing `false` arguments are dropped.  Kernels only in
NEW are listed as new.  Exit status 1 when a matched kernel differs in VGPRs,
AGPRs, SGPRs, scratch, occupancy, spills or LDS.
"""
import re
import subprocess
import sys

KEYS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill",
        "VGPRs Spill", "LDS Size [bytes/block]"]
SHORT = ["VGPR", "AGPR", "SGPR", "scratch", "occ", "SGPR spill", "VGPR spill", "LDS"]


def strip_params(name):
    """A demangled function name without its trailing parameter list.  (Not by a greedy pattern from the first
    parenthesis: an enum template argument is spelled with one, "(mck::MsgFrame)3".)"""
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        depth += (name[i] == ")") - (name[i] == "(")
        if depth == 0:
            return name[:i] if name.endswith(")") else name
    return name


def parse(path):
    rows, cur = {}, None
    for line in open(path):
        m = re.search(r"(?:remark: )?\S+:\d+:\d+: (?:remark: )?(.*?) \[-Rpass", line)
        if not m:
            continue
        txt = m.group(1).strip()
        if txt.startswith("Function Name:"):
            name = subprocess.run(["c++filt", txt.split(":", 1)[1].strip()], capture_output=True, text=True).stdout.strip()
            name = strip_params(re.sub(r"\(anonymous namespace\)::|^void ", "", name))
            cur = rows.setdefault(name, {})
        elif cur is not None and ":" in txt:
            k, v = txt.split(":", 1)
            cur[k.strip()] = v.strip()
    return rows


def older_names(name):
    yield name
    while re.search(r", false>$", name):
        name = re.sub(r", false>$", ">", name)
        yield name


def main():
    md = "--markdown" in sys.argv
    old, new = (parse(p) for p in [a for a in sys.argv[1:] if not a.startswith("--")][:2])
    bad, seen = 0, set()
    sep = " | " if md else "  "
    print(sep.join(["kernel".ljust(58)] + [s.rjust(10) for s in SHORT] + ["vs old"]))
    if md:
        print(sep.join(["---"] * (len(SHORT) + 2)))
    for name, r in new.items():
        match = next((n for n in older_names(name) if n in old), None)
        vals = [str(r.get(k, "-")) for k in KEYS]
        if match is None:
            verdict = "new"
        else:
            seen.add(match)
            ov = [str(old[match].get(k, "-")) for k in KEYS]
            verdict = "same" if ov == vals else "DIFFERS (old: " + " ".join(ov) + ")"
            bad += ov != vals
        print(sep.join([name.ljust(58)] + [v.rjust(10) for v in vals] + [verdict]))
    for name in old:
        if name not in seen:
            print(f"{name}: only in the old log")
            bad += 1
    print(f"{len(seen)} kernels matched, {bad} differ or are missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
