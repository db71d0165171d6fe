"""Record what every plan of tests/plan_cases.py is named, which kernel its execute launches and the SHA-256 of its output:

    python tests/golden/make_plan_golden.py [OUT.json]        (default: tests/golden/plan_routes.json; needs the GPU)

Run on the commit whose behaviour is to be kept -- tests/test_gpu_plan_lifecycle.py holds later commits to the file name for name and bit
for bit.  Run it twice and compare: a case whose two recordings differ in hash is not reproducible and keeps its names only
(--merge A.json B.json OUT.json writes that).  Imports the package alone, never the oracle."""
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
            assert a[name][:2] == b[name][:2], name
            if a[name][2] != b[name][2]:
                print("not reproducible, names only:", name)
                a[name][2] = None
        out = argv[3]
    else:
        import plan_cases
        a = {}
        for name in plan_cases.CASES:
            a[name] = list(plan_cases.record(name))
            print(name, *a[name], flush=True)
        out = argv[0] if argv else os.path.join(HERE, "plan_routes.json")
    with open(out, "w") as f:
        json.dump(a, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
