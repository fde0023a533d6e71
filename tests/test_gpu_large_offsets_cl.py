"""The channels-last BatchNorm site with x and y just past 2^31 elements, through the C ABI of the gfx950 build
(tests/large_cases_cl.py: the cases; tests/large_cases.py: the replicated pool and the checker; tests/test_cl_cpu.py holds the
cases to the pool's premises and teeth on the CPU).  A case allocates about 17 GB and takes a few seconds; it skips only if the
device has less free memory than its peak plus 4 GiB."""
import json

import pytest

import large_cases as lc
import large_cases_cl as lccl
from test_gpu_parity import api, dev  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", lccl.CASES, ids=repr)
def test_large_offsets(api, dev, case):
    res = lc.run_on_device(case, api, dev, pytest.skip)
    assert "y" in res["ratios"] and max(res["ratios"].values()) <= 1.0, res
    print("LARGE " + json.dumps({"case": case.name, "peak_bytes": res["peak"], "allocated_peak_bytes": res["measured_peak"],
                                 "seconds": round(res["seconds"], 2), "worst_ratio": {k: round(v, 4) for k, v in res["ratios"].items()}}))
