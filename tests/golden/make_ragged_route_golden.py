"""Record which kernel every batch of tests/ragged_route_cases.py launches and the SHA-256 of its output arena:

    python tests/golden/make_ragged_route_golden.py [OUT.json]        (default: tests/golden/ragged_routes.json; needs the GPU)

Run on the commit whose behaviour is to be kept -- tests/test_gpu_ragged_routes.py holds later commits to the file name for name and hash for
hash, tests/test_routes_host.py holds zafx_routes.hpp to the names and to the last two entries: the `aligned` flag of a native forward launch
and whether the int16 launch takes an integer batch, restated from that commit's conditions (ragged_route_cases.expected_aligned, pcm_taken).
Run it twice and compare: a case whose two recordings differ in hash is not reproducible and keeps its name only (--merge A.json B.json
OUT.json writes that).  A call the library refuses is recorded as ["refused", the message, null, null].  Imports the package alone, never
the oracle."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "zaf-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv):
    if argv[:1] == ["--merge"]:
        a, b = (json.load(open(p)) for p in argv[1:3])
        assert list(a) == list(b)
        for name in a:
            assert a[name][0] == b[name][0] and a[name][2:] == b[name][2:], name
            if a[name][1] != b[name][1]:
                print("not reproducible, name only:", name)
                a[name][1] = None
        out = argv[3]
    else:
        import ragged_route_cases
        a = {}
        for name in ragged_route_cases.CASES:
            a[name] = list(ragged_route_cases.record(name))
            print(name, *a[name], flush=True)
            if a[name][0] == "refused" and "hip" in a[name][1].lower():   # (a device error is no refusal: nothing more runs on that device)
                sys.exit(f"{name}: {a[name][1]}")
        out = argv[0] if argv else os.path.join(HERE, "ragged_routes.json")
    with open(out, "w") as f:
        json.dump(a, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
