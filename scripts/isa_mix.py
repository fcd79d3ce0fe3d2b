#!/usr/bin/env python3
"""Instruction mix of a kernel's largest loop, from `hipcc -S` output.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -S \
        --cuda-device-only jacobi3d_tbr.hip -o tbr.s
    python scripts/isa_mix.py tbr.s 'jacobi3d_tbrILi4ELi11ELi2ELb1ELi1ELi0ELi0ELb0E'

The kernel is the first symbol whose (mangled) name contains the given text.
A loop is the span from a label to the last backward branch that targets it;
the largest span by instruction count is taken as the kernel's main loop (the
z-march of the temporal-blocking kernels).  Opcodes are tallied by their name
alone: the `v_*` and `ds_*` ones one by one, everything else by the prefix up
to the first underscore.  Encoding suffixes (_e32, _e64, _dpp, _sdwa) are
dropped, so `v_add_f32_e32` and `v_add_f32_dpp` count as `v_add_f32`, with the
DPP forms also summed under `(dpp)`.
"""
from __future__ import annotations

import argparse
import collections
import re
import sys

LABEL = re.compile(r"^([.\w$]+):")
SUFFIX = re.compile(r"_(e32|e64|dpp|sdwa|e64_dpp)$")


def kernel_lines(text: list[str], name: str) -> tuple[str, list[str]]:
    start = sym = None
    for i, line in enumerate(text):
        m = LABEL.match(line)
        if m and name in m.group(1) and not m.group(1).startswith("."):
            start, sym = i + 1, m.group(1)
            break
    if start is None:
        raise SystemExit(f"no kernel symbol contains {name!r}")
    body = []
    for line in text[start:]:
        if line.lstrip().startswith((".end_amdhsa_kernel", ".Lfunc_end", ".section")):
            break
        body.append(line)
    return sym, body


def instructions(body: list[str]):
    """(label or None, opcode or None, operands) per line that is either."""
    for line in body:
        code = line.split(";", 1)[0].rstrip()
        m = LABEL.match(code)
        if m:
            yield m.group(1), None, ""
            continue
        code = code.strip()
        if not code or code.startswith("."):
            continue
        parts = code.split(None, 1)
        yield None, parts[0], parts[1] if len(parts) > 1 else ""


def largest_loop(items):
    label_at = {}
    best = (0, 0, 0)  # instructions, first, last
    n_before = []
    n = 0
    for lab, op, _ in items:
        n_before.append(n)
        if op:
            n += 1
    for i, (lab, op, args) in enumerate(items):
        if lab:
            label_at[lab] = i
        elif op.startswith(("s_cbranch", "s_branch")):
            tgt = args.strip()
            if tgt in label_at:  # backward branch: a loop from the label to here
                size = n_before[i] + 1 - n_before[label_at[tgt]]
                if size > best[0]:
                    best = (size, label_at[tgt], i)
    return best


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm", help="assembly file written by hipcc -S")
    ap.add_argument("kernel", help="text contained in the kernel's mangled name")
    ap.add_argument("--whole", action="store_true", help="tally the whole kernel, not its largest loop")
    a = ap.parse_args()
    with open(a.asm) as f:
        sym, body = kernel_lines(f.read().splitlines(), a.kernel)
    items = list(instructions(body))
    size, first, last = largest_loop(items)
    if a.whole or size == 0:
        first, last = 0, len(items) - 1
    detail = collections.Counter()
    groups = collections.Counter()
    for lab, op, _ in items[first:last + 1]:
        if not op:
            continue
        base = SUFFIX.sub("", op)
        if op.startswith(("v_", "ds_")):
            detail[base] += 1
            groups["v_*" if op.startswith("v_") else "ds_*"] += 1
            if op.endswith("_dpp"):
                groups["(dpp)"] += 1
        else:
            groups[op.split("_", 1)[0] + "_*"] += 1
    total = sum(1 for _, op, _ in items[first:last + 1] if op)
    print(f"kernel {sym}")
    print(f"{'whole kernel' if a.whole or size == 0 else 'largest loop'}: {total} instructions")
    for k, v in sorted(groups.items(), key=lambda kv: (-kv[1], kv[0])):
        print(f"  {k:<12} {v}")
    for k, v in sorted(detail.items(), key=lambda kv: (-kv[1], kv[0])):
        print(f"    {k:<28} {v}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
