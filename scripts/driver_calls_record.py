"""usage: python scripts/driver_calls_record.py [OUT.json]
Records tests/golden/driver_calls.json (default OUT), the fixture of tests/test_driver_calls_cpu.py: for every case of
tests/driver_calls.py the backend calls a SimulationSession makes behind the recording stand-in (method and argument digests), the
lines it prints and the keys of the results it returns, next to the digests of the two coarse meshes and the hash of the commit the
tree stands at.  No GPU is needed.  Run it at the commit whose behaviour is to be pinned: the committed file comes from the commit
before the drivers were folded onto ProblemSpec, with a clean working tree but for the three files of the pin themselves."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import driver_calls

    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    out = {"commit": commit, "meshes": driver_calls.mesh_digests(), "transcripts": driver_calls.transcripts()}
    path = sys.argv[1] if len(sys.argv) > 1 else driver_calls.GOLDEN
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(out['transcripts'])} transcripts, {sum(len(t) for t in out['transcripts'].values())} entries at {commit}")


if __name__ == "__main__":
    main()
