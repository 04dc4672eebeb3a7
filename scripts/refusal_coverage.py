"""Which `fail(` sites of a range of lines of a C-API source file have a recorded refusal?

    python scripts/refusal_coverage.py SOURCE FIRST LAST TABLE.json [FUNCTION=entry,entry ...]

Every `fail(TVR_ERR_*, "format", ...)` in lines FIRST..LAST of SOURCE is turned into a pattern (its format with the conversions as wildcards) and matched against the
messages of TABLE.json's rows (entry point, case, status, message).  A site inside an entry point counts only rows of that entry point; a site inside a static helper
counts rows of the entry points named for it (FUNCTION=...), of any entry point otherwise.  Prints the sites without a row; exit status 1 if there are any.
profiles/train_api_split.txt: SOURCE = the parent commit's csrc/tvr_api.hip, lines 1000 1717, tests/golden/train_api_errors.json."""
import json
import re
import sys


def main(source, first, last, table, *reach):
    lines = open(source, encoding="utf-8").read().split("\n")
    first, last = int(first), int(last)
    text = "\n".join(lines[first - 1:last])
    rows = json.load(open(table, encoding="utf-8"))
    entry_points = {r[0] for r in rows}
    callers = {k: v.split(",") for k, v in (a.split("=") for a in reach)}
    head = re.compile(r"^(?:static )?(?:int|size_t) (\w+)\(")
    missing, n = [], 0
    for m in re.finditer(r"fail\(\s*TVR_ERR_\w+,\s*", text):
        i, fmt = m.end(), ""
        while True:
            lit = re.match(r'\s*"((?:[^"\\]|\\.)*)"', text[i:])
            if not lit:
                break
            fmt += lit.group(1)
            i += lit.end()
        line = first + text[:m.start()].count("\n")
        k = line - 1
        while not head.match(lines[k]):
            k -= 1
        fn = head.match(lines[k]).group(1)
        who = callers.get(fn, [fn] if fn in entry_points else sorted(entry_points))
        rx = re.compile("^" + re.sub(r"%(?:zu|lld|d|g|s|u)", ".*", re.escape(fmt).replace("\\%", "%")) + "$", re.S)
        n += 1
        if not any(r[0] in who and rx.match(r[3]) for r in rows):
            missing.append((line, fn, fmt))
    print(f"{n} fail( sites in lines {first}-{last} of {source}; {n - len(missing)} have a recorded row; {len(missing)} have none")
    for line, fn, fmt in missing:
        print(f"  line {line} ({fn}): {fmt[:140]}")
    return 1 if missing else 0


if __name__ == "__main__":
    if len(sys.argv) < 5:
        sys.exit(__doc__)
    sys.exit(main(*sys.argv[1:]))
