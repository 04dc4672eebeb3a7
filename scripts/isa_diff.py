#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 code in two builds of libtvr.so.

For every kernel name: identical / differs / only in OLD / only in NEW.  Compared are the instruction list (isa_check.disassemble) and the
kernel's resource metadata from the code object's notes.  isa_check names branch targets after absolute addresses, which move when a kernel
in front of them is added or removed, so the labels are renumbered per kernel in order of appearance; nothing else is normalised.
Exit status 1 on any `differs` or `only in NEW`.

usage: isa_diff.py OLD.so NEW.so [OLD_KERNEL=NEW_KERNEL ...]
Each further argument names a kernel of OLD and the kernel of NEW that took its place under another (mangled) name — a template that gained a parameter —
and is compared like a pair of equal names: `renamed identical` / `renamed differs`.  They count for the exit status like the others.
"""
import hashlib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_check  # noqa: E402

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")


def renumber(ins):
    """`.LA<addr>` -> `.L<n>`, n counting the labels of this kernel in order of first appearance."""
    names = {}
    return [re.sub(r"\.LA[0-9a-f]+", lambda m: names.setdefault(m.group(0), f".L{len(names)}"), x) for x in ins]


def metadata(path):
    """-> {kernel name: {key: value}} for the keys of META (isa_check.metadata reads the code objects' notes)."""
    return {k: {key: v.get(key) for key in META} for k, v in isa_check.metadata(path).items()}


def load(path):
    ks = {k: renumber(v) for k, v in isa_check.disassemble(path).items()}
    md = metadata(path)
    missing = [k for k in ks if k not in md]
    if missing:
        sys.exit(f"{path}: no metadata note for {missing[:3]}")
    return ks, md


def main(old, new, renamed=()):
    (ko, mo), (kn, mn) = load(old), load(new)
    for tag, p, ks in (("OLD", old, ko), ("NEW", new, kn)):
        print(f"{tag} {p}  sha256 {hashlib.sha256(open(p, 'rb').read()).hexdigest()}  kernels {len(ks)}  instructions {sum(len(v) for v in ks.values())}")
    bad = 0
    count = {"identical": 0, "differs": 0, "only in OLD": 0, "only in NEW": 0}
    for k in sorted(set(ko) | set(kn)):
        if k not in kn:
            verdict = "only in OLD"
        elif k not in ko:
            verdict = "only in NEW"
        elif ko[k] == kn[k] and mo[k] == mn[k]:
            verdict = "identical"
        else:
            verdict = "differs"
            if ko[k] != kn[k]:
                first = next((i for i, (a, b) in enumerate(zip(ko[k], kn[k])) if a != b), min(len(ko[k]), len(kn[k])))
                verdict += f" (instructions {len(ko[k])} -> {len(kn[k])}, first at {first})"
            if mo[k] != mn[k]:
                verdict += " (metadata " + ", ".join(f"{key} {mo[k][key]} -> {mn[k][key]}" for key in META if mo[k][key] != mn[k][key]) + ")"
        count[verdict.split(" (")[0]] += 1
        bad += verdict.startswith(("differs", "only in NEW"))
        print(f"{verdict:12s} {k}")
    print("  ".join(f"{v} {k}" for k, v in count.items()))
    for pair in renamed:
        a, b = pair.split("=")
        if a not in ko or b not in kn:
            sys.exit(f"{pair}: no such kernel in {'OLD' if a not in ko else 'NEW'}")
        same = ko[a] == kn[b] and mo[a] == mn[b]
        bad += not same
        print(f"renamed {'identical' if same else 'differs'} (instructions {len(ko[a])} -> {len(kn[b])}; metadata {'equal' if mo[a] == mn[b] else 'differs'})  {a}  ->  {b}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) < 3 or not all("=" in a for a in sys.argv[3:]):
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
