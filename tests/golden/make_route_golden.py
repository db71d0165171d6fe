"""Record which kernel every call of tests/route_cases.py launches and the SHA-256 of its output:

    python tests/golden/make_route_golden.py [OUT.json]        (default: tests/golden/call_routes.json; needs the GPU)

Run on the commit whose behaviour is to be kept -- tests/test_gpu_routes.py holds later commits to the file name for name and hash for
hash.  Run it twice and compare: a case whose two recordings differ in hash is not reproducible and keeps its name only
(--merge A.json B.json OUT.json writes that).  A call the library refuses is recorded as ["refused", the message].  Imports the package
alone, never the oracle."""
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
            assert a[name][0] == b[name][0], name
            if a[name][1] != b[name][1]:
                print("not reproducible, name only:", name)
                a[name][1] = None
        out = argv[3]
    else:
        import route_cases
        a = {}
        for name in route_cases.CASES:
            a[name] = list(route_cases.record(name))
            print(name, *a[name], flush=True)
        out = argv[0] if argv else os.path.join(HERE, "call_routes.json")
    with open(out, "w") as f:
        json.dump(a, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
