"""Writes tests/agg_route_table.json (the cells of tests/agg_route_cells.py) from the library that is loaded, or dumps every cell
with its kernel instantiation, null counts and output checksums - the A/B of two builds (`BOWGPU_LIB=<path>`): two dumps of equal
libraries are equal byte for byte.

    python scratch/agg_route_table.py write <out.json>      (a routing change on purpose: run at the commit BEFORE a refactor, or after the change)
    python scratch/agg_route_table.py dump <out.txt>
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import agg_route_cells as cells  # noqa: E402


def main():
    mode, path = sys.argv[1], sys.argv[2]
    small = cells.Data(max(cells.rows_n(r) for r in set(cells.ROWS) | set(cells.ROWS_VARIANTS)))
    big = None
    names, table, lines = [], {}, []
    t0 = time.perf_counter()
    for col, rows in cells.groups():
        if rows == "big" and big is None:
            big = cells.Data(cells.BIG_N)
        d = big if rows == "big" else small
        for suffix, n, interval, variants in cells.group_shapes(rows):
            for variant in variants:
                key = "%s|%s|%s" % (col, suffix, variant)
                row = []
                for reducers in cells.REDUCER_SETS:
                    if mode == "dump":
                        code, text = cells.run_cell(d, col, n, interval, variant, reducers, names, detail=True)
                        lines.append("%s|%s %s %s" % (key, "+".join(reducers), cells_describe(code, names), text))
                    else:
                        code = cells.run_cell(d, col, n, interval, variant, reducers, names)
                    row.append(code)
                table[key] = row
    print("%d cells in %.1f s" % (len(table) * len(cells.REDUCER_SETS), time.perf_counter() - t0), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        if mode == "dump":
            f.write("\n".join(lines) + "\n")
        else:
            f.write("{\n\"names\": %s,\n\"reducer_sets\": %s,\n\"cells\": {\n" % (json.dumps(names), json.dumps([list(s) for s in cells.REDUCER_SETS])))
            f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in table.items()))
            f.write("\n}\n}\n")


def cells_describe(code, names):
    if code < 0:
        return "error=%d" % -code
    return "%s long=%s slow=%d" % (names[code // 6], ("none", "all", "some")[code // 2 % 3], code & 1)


if __name__ == "__main__":
    main()
