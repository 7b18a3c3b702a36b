#!/usr/bin/env python3
"""Pairs the batch kernels of two builds of mchecksum_gpu.hip by what they are
-- (width, lanes, mode, operation, NT, light, split) -- instead of by name, and
compares each pair: registers, scratch, LDS, occupancy, code size and the
instruction stream.  For a change that renames the kernels' template
parameters and must leave their machine code alone.

Each build is a directory holding what `make asm` leaves: resource_usage.txt
and the device assembly mchecksum_gpu-hip-amdgcn-amd-amdhsa-gfx950.s.

usage: batch_kernel_pairs.py [--added REGEX] [--asm FILE] OLD_DIR NEW_DIR

--added REGEX: functions of the new build alone whose name matches are listed
with their resources as "added" and do not count against the pairing (a change
that adds kernels and must leave every existing one alone).

--asm FILE: the device assembly's file name in both directories, for a build
of another source file (mchecksum_gpu_ext-hip-amdgcn-amd-amdhsa-gfx950.s: the
segment, core-header and XDR kernels, all paired by name; a kernel whose
template gained trailing defaulted parameters pairs with the old build's kernel
of the name it has once trailing `false` arguments are dropped).

A kernel's key is read from its demangled template arguments, in either
spelling: crc32c_batch_kernel<LOG2G, MODE, VERIFY, NT, LIGHT, SEED, SEAL, COPY>
and crc64_batch_kernel<LOG2G, MODE, VERIFY, NT, SPLIT, SEED> (bool packs), or
<LOG2G, MODE, OP, NT, LIGHT> and <LOG2G, MODE, OP, NT, SPLIT> (BatchOp,
launch_plan.h), or <LOG2G, MODE, OP, NT, LIGHT, DETACHED[, RPC]> (two bools),
or <LOG2G, MODE, OP, NT, LIGHT, FRAME> (MsgFrame, launch_plan.h: the enum's
type is part of the demangled name, "(mck::MsgFrame)3", which tells it from the
bool spelling), or <LOG2G, MODE, OP, NT, LIGHT, FRAME, LIST> (a bool behind the
MsgFrame: the message side by address list, "verify_rpc_list"), or <..., FRAME,
LIST, BOTH> (a second bool: both sides of a detached call by address list,
"verify_detached_both").  In these a detached kernel's operation reads
"verify_detached" / "seal_detached" and a whole-RPC kernel's "verify_rpc" /
"seal_rpc" / "pack_rpc" / "unpack_rpc", so both spellings pair by what a kernel
is.  Exit status 1 unless the pairing is one to one and every pair is equal in
everything.
"""
import hashlib
import os
import re
import subprocess
import sys

from resource_diff import KEYS, older_names, parse, strip_params

OPS = ["checksum", "verify", "update", "seal", "pack", "unpack"]
MODES = ["aligned", "generic", "offsets"]
ASM = "mchecksum_gpu-hip-amdgcn-amd-amdhsa-gfx950.s"


def key_of(name):
    """(width, lg, mode, op, nt, light, split) of a demangled batch kernel name, else None."""
    m = re.search(r"crc(32c|64)_batch_kernel<([^>]*)>", name)
    if not m:
        return None
    width = 32 if m.group(1) == "32c" else 64
    raw = [t.strip() for t in m.group(2).split(",")]
    a = [{"true": 1, "false": 0}.get(t, t) for t in raw]
    a = [int(re.sub(r"^\(.*\)", "", t)) if isinstance(t, str) else t for t in a]
    lg, mode = a[0], a[1]
    if len(a) == 5 or (len(a) in (6, 7, 8) and width == 32):  # <LOG2G, MODE, OP, NT, LIGHT or SPLIT[, DETACHED[, RPC] or FRAME]>
        op, nt, last = a[2], a[3], a[4]
        light, split = (last, 0) if width == 32 else (0, last)
        if len(a) >= 6 and "MsgFrame" in raw[5]:  # MsgFrame: payloads (in place is a run-time field), -, detached, RPC
            frame = ["", None, "_detached", "_rpc"][a[5]]
            if len(a) >= 7 and a[6]:  # LIST: the message side by address list
                frame += "_list"
            if len(a) == 8 and a[7]:  # BOTH: the payloads and the slots of a detached call by address list
                frame += "_both"
            return (width, lg, MODES[mode], OPS[op] + frame, nt, light, split)
        if len(a) >= 6 and a[5]:  # DETACHED: the slot of a verify or a seal in another buffer
            return (width, lg, MODES[mode], OPS[op] + "_detached", nt, light, split)
        if len(a) == 7 and a[6]:  # RPC: whole RPC messages, header and flags with the payload
            return (width, lg, MODES[mode], OPS[op] + "_rpc", nt, light, split)
    else:  # the bool packs
        verify, nt = a[2], a[3]
        if width == 32:
            light, seed, seal, copy = a[4:8]
            split = 0
        else:
            split, seed = a[4:6]
            light = seal = copy = 0
        op = 2 if seed else 4 if seal and copy else 3 if seal else 5 if verify and copy else 1 if verify else 0
    return (width, lg, MODES[mode], OPS[op], nt, light, split)


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def streams(path):
    """Per function of a device .s file: (sha1 of its instruction stream, instruction count, code bytes)."""
    body, name, last, out = None, None, None, {}
    for line in open(path, errors="replace"):
        if body is None:
            m = re.match(r"\s*\.type\s+([^,]+),@function", line)
            if m:
                name, body = m.group(1), []
            elif last and "codeLenInByte" in line:
                out[last][2] = int(line.split("=")[1])
                last = None
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = [hashlib.sha1("\n".join(body).encode()).hexdigest()[:16], sum(not s.endswith(":") for s in body), None]
            last, body = name, None
            continue
        s = line.split(";")[0].strip()
        # directives (debug line information among them) and temporary labels are no instructions
        if not s or (s.startswith(".") and not re.match(r"\.LBB\d+_\d+:", s)) or re.match(r"\.?Ltmp\d+:", s):
            continue
        s = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s)
        # the kernels' names carry their template arguments (a kernel's own label is part of its stream)
        s = re.sub(r"\b_Z\w*(?:_batch_kernel|xdr_rpc_kernel|xdr_rpc_fast_kernel)\w*", "SYMBOL", s)
        body.append(s)
    return out


def load(d, asm_name=ASM):
    res = parse(os.path.join(d, "resource_usage.txt"))  # keyed by demangled name
    asm = streams(os.path.join(d, asm_name))
    names = demangle(list(asm))
    rows = {}
    for mangled, (sha, n, size) in asm.items():
        short = re.sub(r"\(anonymous namespace\)::|^void ", "", names[mangled])
        k = key_of(short)
        if k is None:  # the element kernels and the device functions the batch kernels call: by name
            short = strip_params(short)
            k = (0, 0, "-", short, 0, 0, 0)
        elif not short.startswith("crc"):  # a function one batch kernel did not inline: by that kernel and its own name
            k = k + (short.split("<")[0],)
        else:
            short = strip_params(short)
        if k in rows:
            sys.exit(f"{d}: two functions with key {k}")
        rows[k] = dict(sha=sha, insts=n, code=size, res=[res.get(short, {}).get(x, "-") for x in KEYS])
    return rows


def main():
    args = sys.argv[1:]
    added = None  # --added REGEX: functions expected in the new build only (a change that adds kernels and must leave the rest alone)
    if "--added" in args:
        i = args.index("--added")
        added = re.compile(args[i + 1])
        del args[i:i + 2]
    asm_name = ASM
    if "--asm" in args:
        i = args.index("--asm")
        asm_name = args[i + 1]
        del args[i:i + 2]
    old, new = load(args[0], asm_name), load(args[1], asm_name)
    # A kernel paired by name whose template gained trailing defaulted parameters (xdr_rpc_kernel<OP> became
    # xdr_rpc_kernel<OP, LIST = false>): the new build's "<..., false>" is the old build's kernel of the shorter name.
    for k in [k for k in new if k not in old and k[2] == "-"]:
        for name in list(older_names(k[3]))[1:]:
            ko = k[:3] + (name,) + k[4:]
            if ko in old and ko not in new:
                new[ko] = new.pop(k)
                break
    bad = nadded = 0
    print("width lanes mode operation nt light split | " + " | ".join(KEYS) + " | code bytes | instructions | stream sha1 | verdict")
    for k in sorted(set(old) | set(new)):
        label = f"{k[0]} {1 << k[1]} {k[2]} {k[3]} {k[4]} {k[5]} {k[6]}" + (f" ({k[7]}, not inlined)" if len(k) > 7 else "")
        if added and k not in old and added.search(str(k[3])):
            n = new[k]
            print(f"{label} | " + " | ".join(n["res"]) + f" | {n['code']} | {n['insts']} | {n['sha']} | added")
            nadded += 1
            continue
        if k not in old or k not in new:
            print(f"{label} | only in the {'new' if k in new else 'old'} build")
            bad += 1
            continue
        o, n = old[k], new[k]
        same = o["res"] == n["res"] and o["code"] == n["code"] and o["sha"] == n["sha"] and o["code"] is not None
        bad += not same
        print(f"{label} | " + " | ".join(n["res"]) + f" | {n['code']} | {n['insts']} | {n['sha']} | " +
              ("same" if same else f"DIFFERS (old: {' '.join(o['res'])} | {o['code']} | {o['insts']} | {o['sha']})"))
    print(f"{len(old)} kernels in the old build, {len(new)} in the new, {len(set(old) & set(new))} paired, "
          + (f"{nadded} added, " if added else "") + f"{bad} differ or are unpaired")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
