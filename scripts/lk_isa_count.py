#!/usr/bin/env python3
"""Static instruction counts of the Lucas-Kanade kernels (flvis_amd/csrc/lk_kernel.hip).

Compiles the file to gfx950 assembly with the flags of flvis_amd/build.py (device side only, into a temporary directory) and prints, for
each of the three kernels (and for the out-of-line template function the temporal launch calls), the instruction counts of the level
set-up and of the iteration loop, block by block.  Instructions are classed by opcode prefix only:

    vector  v_*            scalar  s_* (what is not listed below)     lds   ds_*
    memory  global_* flat_* buffer_* scratch_* s_load_* s_buffer_load_*
    wait    s_waitcnt*     no-op   s_nop     branch  s_branch s_cbranch_* s_setpc_* s_swappc_* s_call_* s_endpgm

The loops are the compiler's own (the `in Loop: Header=... Depth=...` comments of the listing): the iteration loop is the loop of depth 3
(point, level, iteration) around the largest block that lies that deep.  It holds the position and region tests, the re-staging of the
search region (taken when the window has left the staged region), the pixel loop, the wave sum and the update with its exit tests; a
loop inside it (the index-reflecting staging next to an image edge) is left out of the second total.
It is a counter, not a checker: it asserts nothing about the counts.  The launches are bound by instruction issue (one instruction of any
class per 4 cycles and SIMD: profiles/r06_chain_ab.md), so these counts are what a change to the kernel is weighed by before it is timed.

    python scripts/lk_isa_count.py [--source FILE] [--blocks] [--keep DIR] [--markdown]
"""
import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = ("vector", "scalar", "lds", "memory", "wait", "no-op", "branch")
KERNELS = ("k_lk_track_temporal", "k_lk_track_stereo", "k_lk_track")


def classify(op):
    if op == "s_nop":
        return "no-op"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith(("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_call", "s_endpgm")):
        return "branch"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_", "s_load", "s_buffer_load")):
        return "memory"
    if op.startswith("v_"):
        return "vector"
    if op.startswith("s_"):
        return "scalar"
    return None


def compile_to_asm(source, outdir):
    from flvis_amd import build as B
    out = os.path.join(outdir, "lk_kernel.s")
    cmd = [B.HIPCC] + B.FLAGS + ["--cuda-device-only", "-S", source, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise SystemExit("hipcc failed:\n" + r.stdout.decode(errors="replace"))
    return out


class Block:
    def __init__(self, label):
        self.label = label
        self.ops = []            # opcodes in order
        self.loop = None         # label of the innermost loop's header block, from the compiler's own loop comments
        self.depth = 0           # its depth (1: outermost)
        self.parents = {}        # of a header block: depth -> header label of the loops around it

    def counts(self):
        c = collections.Counter()
        for op in self.ops:
            c[classify(op)] += 1
        return c


def functions(asm_text):
    """-> {symbol: [Block]} for every function of the listing, blocks in layout order.  A block starts at a label or at the `; %bb.N:`
    comment of a block that is only fallen into; the loop each block belongs to is what the compiler's comments say."""
    out, cur, name = {}, None, None
    label_re = re.compile(r"^([A-Za-z_.$][\w.$]*):")
    fall_re = re.compile(r"^; (%bb\.\d+):")
    for raw in asm_text.splitlines():
        m = label_re.match(raw) or fall_re.match(raw)
        if m:
            lab = m.group(1)
            if lab.startswith(".Lfunc_end"):
                name, cur = None, None
                continue
            if lab.startswith((".LBB", "%bb")):
                if name is None:
                    continue
                cur = Block(lab)
                out[name].append(cur)
            elif not lab.startswith("."):
                name = lab
                cur = Block(lab)
                out[name] = [cur]
            else:
                continue
        if cur is not None and ";" in raw:
            note = raw.split(";", 1)[1]
            m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", note)
            if m:
                cur.loop, cur.depth = ".L" + m.group(1), int(m.group(2))
            m = re.search(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", note)
            if m:
                cur.parents[int(m.group(2))] = ".L" + m.group(1)
            m = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", note)
            if m:
                cur.loop, cur.depth = cur.label, int(m.group(1))
        line = raw.split(";")[0].strip()
        if cur is None or not line or label_re.match(line):
            continue
        op = line.split()[0]
        if classify(op) is not None:
            cur.ops.append(op)
    return {k: v for k, v in out.items() if any(b.ops for b in v)}


def total(blocks):
    c = collections.Counter()
    for b in blocks:
        c.update(b.counts())
    return c


def row(name, c):
    return [name, str(sum(c.values()))] + [str(c.get(k, 0)) for k in CLASSES]


def analyse(blocks):
    """-> (rows of the summary, rows per block of the iteration loop).  The iteration loop is the loop of depth 3 (point, level,
    iteration) around the largest block that lies at least that deep; the level loop is the loop of depth 2 around it."""
    by_label = {b.label: b for b in blocks}

    def chain(b):
        """depth -> header label of every loop around block b"""
        if b.loop is None:
            return {}
        c = dict(by_label[b.loop].parents)
        c[b.depth] = b.loop
        return c

    rows, per_block = [row("whole function", total(blocks))], []
    deep = [b for b in blocks if b.depth >= 3]
    if not deep:
        return rows, per_block
    big = max(deep, key=lambda b: len(b.ops))
    it, level = chain(big)[3], chain(big)[2]
    in_level = [b for b in blocks if chain(b).get(2) == level]
    in_it = [b for b in in_level if chain(b).get(3) == it]
    rows.append(row("level loop without the iteration loop (set-up)", total([b for b in in_level if b not in in_it])))
    rows.append(row("iteration loop, every block", total(in_it)))
    rows.append(row("iteration loop without the loops inside it", total([b for b in in_it if b.depth == 3])))
    rows.append(row("iteration loop, its largest block (pixel loop)", big.counts()))
    for b in in_it:
        per_block.append(row(b.label + (" (depth %d)" % b.depth if b.depth > 3 else ""), b.counts()))
    return rows, per_block


def metadata(asm_text):
    """-> {kernel symbol: {vgpr, sgpr, vgpr_spill, sgpr_spill, lds, scratch}} from the amdhsa.kernels notes"""
    keys = {".vgpr_count": "vgpr", ".sgpr_count": "sgpr", ".vgpr_spill_count": "vgpr_spill", ".sgpr_spill_count": "sgpr_spill",
            ".group_segment_fixed_size": "lds", ".private_segment_fixed_size": "scratch", ".name": "name"}
    out, cur = {}, None
    for line in asm_text.splitlines():
        if re.match(r"^  - \.", line):            # a new entry of amdhsa.kernels
            cur = {}
        m = re.match(r"^  (?:- |  )(\.[a-z_]+):\s*(\S+)\s*$", line)      # (the entry's own keys, not those of its .args)
        if cur is None or not m:
            continue
        if m.group(1) in keys:
            cur[keys[m.group(1)]] = m.group(2)
            if "name" in cur:
                out[cur["name"]] = cur
    return out


def table(rows, markdown):
    head = ["part", "all"] + list(CLASSES)
    if markdown:
        lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
        lines += ["| " + " | ".join(r) + " |" for r in rows]
        return "\n".join(lines)
    w = [max(len(r[i]) for r in [head] + rows) for i in range(len(head))]
    fmt = lambda r: "  ".join(c.ljust(w[i]) if i == 0 else c.rjust(w[i]) for i, c in enumerate(r))
    return "\n".join([fmt(head)] + [fmt(r) for r in rows])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--source", default=os.path.join(ROOT, "flvis_amd", "csrc", "lk_kernel.hip"))
    ap.add_argument("--blocks", action="store_true", help="also one row per block of the iteration loop")
    ap.add_argument("--keep", metavar="DIR", help="copy the assembly listing into DIR")
    ap.add_argument("--markdown", action="store_true")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="lk_isa_")
    try:
        text = open(compile_to_asm(a.source, tmp)).read()
        if a.keep:
            os.makedirs(a.keep, exist_ok=True)
            shutil.copy(os.path.join(tmp, "lk_kernel.s"), a.keep)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    fns, meta = functions(text), metadata(text)
    for sym, blocks in fns.items():
        kern = next((k for k in KERNELS if re.search(r"%sE" % k, sym) or sym == k), None)
        if kern is None and "lk_template_level_cold" not in sym:
            continue
        title = kern or "lk_template_level_cold (called by k_lk_track_temporal for a template the cache does not hold)"
        print(("### " if a.markdown else "== ") + title)
        m = meta.get(sym)
        if m:
            print("registers: %s VGPR, %s SGPR; spills: %s VGPR, %s SGPR; LDS %s B, scratch %s B" % (
                m.get("vgpr", "?"), m.get("sgpr", "?"), m.get("vgpr_spill", "?"), m.get("sgpr_spill", "?"), m.get("lds", "?"), m.get("scratch", "?")))
        if a.markdown:
            print()
        rows, per_block = analyse(blocks)
        print(table(rows, a.markdown))
        if a.blocks and per_block:
            print()
            print(table(per_block, a.markdown))
        print()


if __name__ == "__main__":
    main()
