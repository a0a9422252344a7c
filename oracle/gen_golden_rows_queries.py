"""TEST INFRASTRUCTURE (not product code).  Records what the pure-host geometry queries of a BUILT
libsegmentron_hip.so answer (chunk counts, partial rows, row-tile and depthwise grids; no device
needed) over the sweep of tests/_rows_queries.py into tests/golden/rows_queries.json for
tests/test_host_api.py, which replays them against the library under test.  The fixture pins the
move of that arithmetic into csrc/rows.h, so it must come from the build of the commit BEFORE the
move, never from the code under test:
    SEGMENTRON_HIP_LIB=<parent build>/segmentron_amd/libsegmentron_hip.so \
        python oracle/gen_golden_rows_queries.py <parent commit id>
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    if not os.environ.get("SEGMENTRON_HIP_LIB") or len(sys.argv) != 2:
        sys.exit("usage: SEGMENTRON_HIP_LIB=<library of the commit to pin> %s <its commit id>"
                 % sys.argv[0])
    from segmentron_amd import _lib  # (argument types from include/segmentron_hip.h)
    import _rows_queries
    table = _rows_queries.sweep(_lib.LIB.query)
    out = os.path.join(ROOT, "tests", "golden", "rows_queries.json")
    with open(out, "w") as f:
        json.dump({"recorded_from": sys.argv[1], "values": table}, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", out, {k: len(v) for k, v in table.items()})


if __name__ == "__main__":
    main()
