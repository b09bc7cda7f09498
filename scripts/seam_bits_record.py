"""usage (GPU box): python scripts/seam_bits_record.py [OUT.json]
Records tests/golden/seam_bits.json (default OUT), the fixture of tests/test_gpu_seam_bits.py: SHA-256 digests and iteration counts
of the steady, Picard, tangent and read-flux calls on the two small cases, computed by that test's own digests().  Run it with the
library whose bits are to be pinned (HEATFLOW_HIP_LIB selects one); the committed file comes from the library of the commit before
the operator and the batch state became arguments, recorded twice in two processes with the same output.  Prints what it wrote."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    from conftest import build_case
    from heatflow_amd import hip_backend
    from test_gpu_seam_bits import CASES, GOLDEN, GROUPS, digests

    hip_backend.load_library()
    out = {}
    for name in sorted(CASES):
        case = build_case(name, 8.0)
        out[name] = {group: digests(hip_backend, case, group) for group in GROUPS}
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
