"""Host side of libdmel_hip.so under AddressSanitizer on a fake HIP runtime (tools/asan/): packers, re-tilers, table builders, workspace
planners, argument checks and launch assembly of every handle run for real, the kernels do not.  GPU sanitizers are not available on
the pool; this is the CPU-build sanitizer run SURVEY.md section 5 lists.

The same run fingerprints every packed weight image: the driver prints, per module handle, the sorted (byte count, FNV-1a) pairs of all
it uploaded between create and the return of finalize, from fixed-seed pseudo-random weights.  tests/golden/host_image_fingerprints.txt
is that output as recorded BEFORE the weight-image descriptions were unified; it is never regenerated from later code.  A line that
differs means a host packer now writes different bytes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not found")


@pytest.fixture(scope="module")
def asan_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("asan")
    return subprocess.run(["bash", os.path.join(ROOT, "tools", "asan", "run.sh"), str(out)], capture_output=True, text=True, timeout=900)


def test_host_side_is_asan_clean(asan_run):
    r = asan_run
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "no sanitizer report" in r.stdout


def test_packed_images_match_recorded_fingerprints(asan_run):
    with open(os.path.join(ROOT, "tests", "golden", "host_image_fingerprints.txt")) as f:
        want = [l for l in f.read().splitlines() if l]
    got = [l for l in asan_run.stdout.splitlines() if l.startswith("uploads ")]
    assert [l.split(":")[0] for l in got] == [l.split(":")[0] for l in want]       # same handles, same order
    for g, w in zip(got, want):
        assert g == w, "%s: %d of %d uploads differ" % (w.split(":")[0], len(set(g.split()) ^ set(w.split())) // 2, len(w.split()) - 1)
