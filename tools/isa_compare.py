#!/usr/bin/env python3
"""Compare two AMDGPU assembly files (hipcc -S --cuda-device-only) kernel by kernel: what a source-only refactor has to leave alone.

    python tools/isa_compare.py before.s after.s [--ignore-count MNEMONIC ...] [--markdown]

Per kernel symbol (every .amdhsa_kernel block and the function body under the label of the same name) it reports
  - whether the sequence of instruction mnemonics is equal (operands, labels, comments and directives are not compared:
    register allocation may rename, the order of the instructions may not change),
  - the .amdhsa_* values that differ (registers, LDS, scratch, ...),
  - the mnemonics whose counts differ.
Exit status 1 when the symbol sets differ, an .amdhsa_* value differs, or the count of a mnemonic that is not named with
--ignore-count differs; a sequence that differs only in ignored mnemonics is reported and does not fail."""
import argparse
import collections
import re
import sys

LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")


def parse(path):
    """{symbol: {"amdhsa": {key: value}, "insts": [mnemonic, ...]}} of the kernels of one assembly file"""
    amdhsa, bodies = {}, {}
    cur_desc = cur_body = None
    with open(path) as f:
        for raw in f:
            line = raw.split(";", 1)[0].rstrip()
            if not line.strip():
                continue
            m = LABEL.match(line)
            if m:
                name = m.group(1)
                if name.startswith(".Lfunc_end"):
                    cur_body = None
                elif not name.startswith("."):
                    cur_body = bodies.setdefault(name, [])
                continue
            tok = line.split()
            if tok[0] == ".amdhsa_kernel":
                cur_desc = amdhsa.setdefault(tok[1], {})
            elif tok[0] == ".end_amdhsa_kernel":
                cur_desc = None
            elif tok[0].startswith(".amdhsa_") and cur_desc is not None:
                cur_desc[tok[0]] = " ".join(tok[1:])
            elif not tok[0].startswith(".") and cur_body is not None:
                cur_body.append(tok[0])
    return {k: {"amdhsa": v, "insts": bodies.get(k, [])} for k, v in amdhsa.items()}


def compare(a, b, ignore):
    rows, ok = [], set(a) == set(b)
    for sym in sorted(set(a) | set(b)):
        if sym not in a or sym not in b:
            rows.append((sym, None, None, None, "only in " + ("the first" if sym in a else "the second") + " file"))
            continue
        ia, ib = a[sym]["insts"], b[sym]["insts"]
        ha, hb = a[sym]["amdhsa"], b[sym]["amdhsa"]
        dh = {k: (ha.get(k), hb.get(k)) for k in sorted(set(ha) | set(hb)) if ha.get(k) != hb.get(k)}
        ca, cb = collections.Counter(ia), collections.Counter(ib)
        dc = {k: (ca[k], cb[k]) for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k]}
        if dh or any(k not in ignore for k in dc):
            ok = False
        rows.append((sym, ia == ib, dh, dc, "%d / %d instructions" % (len(ia), len(ib))))
    return rows, ok


def fmt(d):
    return ", ".join("%s %s -> %s" % (k, v[0], v[1]) for k, v in d.items()) if d else "none"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--ignore-count", action="append", default=[], metavar="MNEMONIC", help="a count difference of this mnemonic does not fail the comparison")
    ap.add_argument("--markdown", action="store_true", help="print a table")
    args = ap.parse_args()
    rows, ok = compare(parse(args.before), parse(args.after), set(args.ignore_count))
    if args.markdown:
        print("| kernel | sequence | .amdhsa_* differences | mnemonic count differences |\n|---|---|---|---|")
    for sym, same, dh, dc, note in rows:
        if same is None:
            print(("| `%s` | %s | | |" if args.markdown else "%s: %s") % (sym, note))
        elif args.markdown:
            print("| `%s` | %s (%s) | %s | %s |" % (sym, "identical" if same else "differs", note, fmt(dh), fmt(dc)))
        else:
            print("%s\n  sequence %s (%s)\n  amdhsa differences: %s\n  count differences: %s" % (sym, "identical" if same else "DIFFERS", note, fmt(dh), fmt(dc)))
    print(("%d kernels: " % len(rows)) + ("equal symbols, resources and counts" if ok else "DIFFERENT"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
