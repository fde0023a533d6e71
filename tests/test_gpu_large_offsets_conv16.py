"""conv32x1 on a 16-bit x with x and grad_x just past 2^31 elements, through the C ABI of the gfx950 build
(tests/large_cases_conv16.py: the cases; tests/large_cases.py: the replicated pool and the checker; tests/test_mixed_conv_cpu.py
shows on the CPU that wrapped offsets are rejected).  A case allocates about 9 GB and takes a few seconds; it skips only if the
device has less free memory than its peak plus 4 GiB."""
import json

import pytest

import large_cases as lc
import large_cases_conv16 as lc16
from test_gpu_parity import api, dev  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", lc16.CASES, ids=repr)
def test_large_offsets(api, dev, case):
    res = lc.run_on_device(case, api, dev, pytest.skip)
    assert res["ratios"] and max(res["ratios"].values()) <= 1.0, res
    print("LARGE " + json.dumps({"case": case.name, "peak_bytes": res["peak"], "allocated_peak_bytes": res["measured_peak"],
                                 "seconds": round(res["seconds"], 2), "worst_ratio": {k: round(v, 4) for k, v in res["ratios"].items()}}))
