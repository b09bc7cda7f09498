"""The Python drivers' conversation with their backend, pinned call by call (no GPU): SimulationSession.run / prepare / run_batch
behind a recording stand-in (tests/driver_calls.py) must make the backend calls, with the arguments, print the lines and return the
result keys that tests/golden/driver_calls.json holds.  The file was recorded by scripts/driver_calls_record.py at the commit it
names ("commit"), before the drivers were folded onto ProblemSpec, and only the session's public API is used, so
the test reads the same at that commit and after it.

The cases, each on the coarse mesh (every mats.*.mesh times 8) with 3 steps at the configuration's own dt: run() of every file of
cfgs/ but the konopkova stub on a fresh session; one session through run, reuse, a re-valued k, a k beyond the hierarchy's range,
more steps at the same dt and another dt; prepare then run; a shared hierarchy within and beyond its range; read_flux with a field
sink (the step-wise loop); two_sided; the tangent columns of every kind (conductivity, fwhm, k_r / k_z, thickness, capacities,
the source's own, a table's parameter), monitor_tangents and monitor_sigma; run_batch with shared, affine and per-column operators,
beyond the hierarchy's range, under source sweeps, sweep_monitors, sweep_tables, with read_flux, and after a single run under the
source; the latent configuration with its monitors block."""
import json

import pytest

import driver_calls


@pytest.fixture(scope="module")
def golden():
    with open(driver_calls.GOLDEN) as f:
        return json.load(f)


def test_the_meshes_are_the_recorded_ones(golden):
    assert driver_calls.mesh_digests() == golden["meshes"], "the mesher moved: the transcripts below carry other arrays"


def test_every_case_is_recorded(golden):
    assert sorted(golden["transcripts"]) == sorted(driver_calls.CASES)
    assert len(golden["commit"]) == 40


@pytest.mark.parametrize("name", sorted(driver_calls.CASES))
def test_transcript(golden, name):
    got, want = driver_calls.CASES[name](), golden["transcripts"][name]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: entry {k} differs (after {got[max(k - 3, 0):k]})"
    assert len(got) == len(want), f"{name}: {len(got)} entries, {len(want)} recorded; the first extra: {(got + want)[min(len(got), len(want))]}"
