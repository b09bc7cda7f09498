"""usage (GPU box): python scripts/rowgather_bits_record.py [OUT.json]
Records tests/golden/rowgather_bits.json (default OUT), the fixture of tests/test_gpu_rowgather_bits.py: SHA-256 digests of the
mesh arrays and of what each of the ten row-gather assembly kernels writes on the two small cases, computed by that test's own
digests().  Run it with the library whose bits are to be pinned (HEATFLOW_HIP_LIB selects one).  The committed file's entries
of the first seven kernels come from the library of the commit before the kernels were folded into rowgather_assemble; the
*_an entries (tables on anisotropic tags) from the library of the commit before the coefficient policies were folded into
RowsTable, recorded twice in separate processes with the same file both times, and the older entries came out as committed.
Prints the digests it wrote."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    from conftest import build_case
    from heatflow_amd import hip_backend
    from test_gpu_rowgather_bits import CASES, GOLDEN, digests

    hip_backend.load_library()
    out = {name: digests(hip_backend, build_case(name, 8.0)) for name in sorted(CASES)}
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
