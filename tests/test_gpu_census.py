"""What the in-engine sampler enqueues, by the engine's own profile: the launches of every kernel family after one `generate` of 4 steps on
the tiny golden model, in every mode of the tool, against the counts recorded in tests/golden/sampler_census.json (tools/sampler_census.py wrote them).
Bit-identity does not catch a launch enqueued twice or a per-call reset that moved; these counts do.  Profiling turns graph replay off, so
this is the eager loop; the captured step is held by bits in test_gpu_watch.py, test_gpu_edit.py and test_gpu_nag.py."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("k5_sampler_census", os.path.join(ROOT, "tools", "sampler_census.py"))
census = importlib.util.module_from_spec(spec)
spec.loader.exec_module(census)


@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X")
    return census.tiny_model()


def test_census_file_names_every_mode_and_family():
    want = json.load(open(census.CENSUS))
    assert tuple(want) == census.MODES and all(tuple(v) == census.FAMILIES for v in want.values())


@pytest.mark.parametrize("mode", census.MODES)
def test_sampler_enqueues_what_it_did(tiny, mode):
    dit, g = tiny
    got = census.census(dit, g, mode)
    print(mode, got)
    assert got == json.load(open(census.CENSUS))[mode]
    assert got["gemm"] > 0 and got["elementwise"] > 0            # the profile was on
