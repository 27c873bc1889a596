#!/usr/bin/env python3
"""Instruction census of the match scan's chunk loop (pycolmap_amd/csrc/match_mfma.hip).

    python tools/scan_loop_census.py                  # compiles match_mfma.hip with the flags of pycolmap_amd/build.py
    python tools/scan_loop_census.py path/to/file.s   # or reads an assembly file (hipcc -S --cuda-device-only)

For each MODE of match_mfma_kernel it finds the loops that hold the scan's MFMAs and prints, per 128
v_mfma_i32_16x16x64_i8 (one 128-row chunk of Y against a wave's eight X tiles), what else the loop executes: the top-2
work (the algorithm), every other vector instruction by opcode, scalar instructions, branches, s_nop, LDS reads, DMA
instructions and the waits.  The vector pipe is what bounds the scan, so a vector instruction
that forms an address or carries a predicate is what this tool is there to show.

The STEADY loop is the one that also issues the Y stream's DMA (global_load_lds); a loop with MFMAs and no DMA is the
DRAIN of the last chunks.  The `flush` block (every 64 blocks: the basic blocks that set the carried code, `v_or_b32
.., 0x7f, ..`) is counted apart.  VGPRs, scratch and LDS come from the kernel's metadata.
"""
from __future__ import annotations

import json
import re
import subprocess
import sys
import tempfile
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

TOP2 = ("v_max3_i32", "v_max_i32", "v_lshl_or_b32", "v_med3_i32")
_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_FALL = re.compile(r"^; %bb\.\d+:")
_BRANCH = re.compile(r"^\s+(s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)")
_KERNEL = re.compile(r"^(_ZN3amc17match_mfma_kernelILi(\d)E\w+):")
_FLUSH_MARK = re.compile(r"^\s+v_or_b32\w*\s+v\d+, 0x7f, v\d+")


def _opcode(line: str) -> str | None:
    """The mnemonic of an instruction line without its encoding suffix; None for labels, directives and comments."""
    t = line.strip()
    if not t or t[0] in ".;" or t.endswith(":"):
        return None
    op = t.split()[0]
    for suf in ("_e32", "_e64", "_sdwa", "_dpp"):
        if op.endswith(suf):
            op = op[: -len(suf)]
    return op


def _blocks(lines: list[str]) -> list[tuple[int, int]]:
    """Basic blocks of a function body as [start, end) line ranges: cut at labels, fall-through marks and branches."""
    cuts = {0, len(lines)}
    for i, ln in enumerate(lines):
        if _LABEL.match(ln) or _FALL.match(ln):
            cuts.add(i)
        elif _BRANCH.match(ln):
            cuts.add(i + 1)
    edges = sorted(cuts)
    return [(a, b) for a, b in zip(edges, edges[1:]) if a < b]


def _loops(lines: list[str]) -> list[tuple[int, int]]:
    """[header line, back-edge line] of every loop: a branch to a label above it."""
    at = {m.group(1): i for i, ln in enumerate(lines) if (m := _LABEL.match(ln))}
    out = set()
    for j, ln in enumerate(lines):
        m = _BRANCH.match(ln)
        if m and m.group(2) in at and at[m.group(2)] <= j:
            out.add((at[m.group(2)], j))
    # several back edges to one header are one loop: keep the widest
    widest: dict[int, int] = {}
    for a, b in out:
        widest[a] = max(widest.get(a, b), b)
    return sorted(widest.items())


def _count(lines: list[str]) -> dict:
    ops = Counter(op for ln in lines if (op := _opcode(ln)))
    mfma = sum(n for op, n in ops.items() if op.startswith("v_mfma"))
    top2 = {op: ops[op] for op in TOP2 if ops[op]}
    other = {op: n for op, n in ops.items() if op.startswith("v_") and not op.startswith("v_mfma") and op not in TOP2}
    branches = sum(n for op, n in ops.items() if op.startswith("s_cbranch") or op == "s_branch")
    not_salu = ("s_nop", "s_waitcnt", "s_barrier", "s_branch")
    salu = sum(n for op, n in ops.items()
               if op.startswith("s_") and op not in not_salu and not op.startswith("s_cbranch"))
    waits = [" ".join(ln.split()[1:]) for ln in lines if _opcode(ln) == "s_waitcnt"]
    return {
        "mfma": mfma,
        "top2": sum(top2.values()),
        "top2_by_op": top2,
        "other_valu": sum(other.values()),
        "other_valu_by_op": dict(sorted(other.items())),
        "salu": salu,
        "branches": branches,
        "s_nop": ops["s_nop"],
        "ds_read": sum(n for op, n in ops.items() if op.startswith("ds_read")),
        "dma": sum(n for op, n in ops.items() if op.startswith("global_load_lds")),
        "s_barrier": ops["s_barrier"],
        "waits": waits,
    }


def _census_loop(body: list[str], a: int, b: int) -> dict:
    span = body[a:b + 1]
    keep: list[str] = []
    flush: list[str] = []
    for s, e in _blocks(span):
        blk = span[s:e]
        (flush if sum(1 for ln in blk if _FLUSH_MARK.match(ln)) >= 4 else keep).extend(blk)
    c = _count(keep)
    c["flush"] = {k: v for k, v in _count(flush).items() if k in ("other_valu", "other_valu_by_op", "salu")}
    c["kind"] = "steady" if c["dma"] else "drain"
    c["lines"] = [a, b]
    return c


def census(asm: str) -> dict:
    """{mode: {"loops": [...], "vgprs": n, "scratch_bytes": n, "lds_bytes": n}} for the MODEs found in `asm`."""
    lines = asm.splitlines()
    out: dict[int, dict] = {}
    starts = [(i, m.group(1), int(m.group(2))) for i, ln in enumerate(lines) if (m := _KERNEL.match(ln))]
    for i, name, mode in starts:
        end = next((j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end")), len(lines))
        body = lines[i:end]
        loops = _loops(body)
        mfma_loops = [(a, b) for a, b in loops if any("v_mfma" in ln for ln in body[a:b + 1])]
        # innermost: holds no other MFMA loop
        inner = [(a, b) for a, b in mfma_loops
                 if not any((a2, b2) != (a, b) and a <= a2 and b2 <= b for a2, b2 in mfma_loops)]
        k: dict = {"name": name, "loops": [_census_loop(body, a, b) for a, b in inner]}
        meta = _metadata(lines, name)
        k.update(meta)
        out[mode] = k
    return out


def _metadata(lines: list[str], name: str) -> dict:
    keys = {".vgpr_count:": "vgprs", ".private_segment_fixed_size:": "scratch_bytes",
            ".group_segment_fixed_size:": "lds_bytes"}
    # the kernel's entry of amdhsa.kernels: from its `- .agpr_count` (the first key of an entry) to the next one
    at = next((i for i, ln in enumerate(lines) if ln.strip().startswith(".name:") and ln.split()[-1] == name), None)
    if at is None:
        return {}
    lo = at
    while lo > 0 and not lines[lo].lstrip().startswith("- ."):
        lo -= 1
    hi = at
    while hi + 1 < len(lines) and not lines[hi + 1].lstrip().startswith("- .") and not lines[hi + 1].startswith("amdhsa."):
        hi += 1
    got = {}
    for ln in lines[lo:hi + 1]:
        t = ln.replace("- ", "  ", 1).split()
        if len(t) == 2 and t[0] in keys:
            got[keys[t[0]]] = int(t[1])
    return got


def per_chunk(loop: dict) -> dict:
    """A loop's counts scaled to 128 MFMAs."""
    n = loop["mfma"]
    f = (lambda v: v * 128 / n) if n else (lambda v: float("nan"))
    r = {k: f(loop[k]) for k in ("top2", "other_valu", "salu", "branches", "s_nop", "ds_read", "dma", "s_barrier")}
    r["other_valu_by_op"] = {op: f(v) for op, v in loop["other_valu_by_op"].items()}
    r["top2_by_op"] = {op: f(v) for op, v in loop["top2_by_op"].items()}
    return r


def compile_to_asm(out: Path) -> None:
    sys.path.insert(0, str(ROOT))
    from pycolmap_amd import build
    flags = [f for f in build.HIPCC_FLAGS if f != "-fPIC"]
    cmd = [build._hipcc(), *flags, "-S", "--cuda-device-only", str(build.CSRC / "match_mfma.hip"), "-o", str(out),
           f"-I{ROOT / 'include'}"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def _fmt(v: float) -> str:
    return f"{v:g}"


def render(res: dict) -> str:
    rows = []
    for mode in sorted(res):
        k = res[mode]
        rows.append(f"MODE {mode}: VGPRs {k.get('vgprs')}, scratch {k.get('scratch_bytes')} B/lane, "
                    f"LDS {k.get('lds_bytes')} B")
        if not k["loops"]:
            rows.append("  no loop with MFMAs found")
        for lp in k["loops"]:
            p = per_chunk(lp)
            rows.append(f"  {lp['kind']} loop, {lp['mfma']} MFMAs per pass; per 128 MFMAs:")
            rows.append("    top-2 work       " + _fmt(p["top2"]) + "  ("
                        + ", ".join(f"{op} {_fmt(v)}" for op, v in p["top2_by_op"].items()) + ")")
            rows.append("    other VALU       " + _fmt(p["other_valu"]) + "  ("
                        + ", ".join(f"{op} {_fmt(v)}" for op, v in p["other_valu_by_op"].items()) + ")")
            for key, label in (("salu", "SALU"), ("branches", "branches"), ("s_nop", "s_nop"), ("ds_read", "ds_read"),
                               ("dma", "DMA"), ("s_barrier", "s_barrier")):
                rows.append(f"    {label:<16} {_fmt(p[key])}")
            rows.append("    s_waitcnt        " + "; ".join(f"{w} x{n}" for w, n in Counter(lp["waits"]).items()))
            fl = lp["flush"]
            rows.append(f"    flush block (apart): VALU {fl['other_valu']}, SALU {fl['salu']}")
    return "\n".join(rows)


def main(argv: list[str]) -> int:
    as_json = "--json" in argv
    args = [a for a in argv if a != "--json"]
    if args:
        asm = Path(args[0]).read_text()
    else:
        with tempfile.TemporaryDirectory() as td:
            out = Path(td) / "match_mfma.s"
            compile_to_asm(out)
            asm = out.read_text()
    res = census(asm)
    print(json.dumps(res, indent=1) if as_json else render(res))
    return 0 if res and all(k["loops"] for k in res.values()) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
