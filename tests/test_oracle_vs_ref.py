"""Pins the C restatement against the reference's own kernel bodies on seeded random inputs, including awkward shapes.
The reference's outputs on these cases were computed by oracle/_ref (built by oracle/Makefile) and are committed with
their inputs in tests/golden/vs_ref_golden.npz (tests/golden/make_golden.py --vs-ref)."""
import pytest

import golden_util as gu
from golden_util import assert_bit_equal, load


@pytest.mark.parametrize("shape", gu.VS_REF_SGA_SHAPES)
def test_sga_port_equals_reference(port_oracle, shape):
    z, k = load("vs_ref_golden.npz"), gu.vs_ref_key("sga", shape)
    x, go = z[f"{k}.x"], z[f"{k}.go"]
    gs = [z[f"{k}.g{d}"] for d in range(4)]
    a = port_oracle.sga_forward(x, *gs)
    for u, n in zip(a, ("out", "temp_out", "mask")):
        assert_bit_equal(u, z[f"{k}.{n}"], n)
    ga = port_oracle.sga_backward(x, *gs, a[1], a[2], go)
    for u, n in zip(ga, ("gx", "gw0", "gw1", "gw2", "gw3")):
        assert_bit_equal(u, z[f"{k}.{n}"], n)


@pytest.mark.parametrize("shape,r", gu.VS_REF_LGA_CASES)
def test_lga_port_equals_reference(port_oracle, shape, r):
    z, k = load("vs_ref_golden.npz"), gu.vs_ref_key("lga", shape, r)
    x, f, gy = z[f"{k}.x"], z[f"{k}.f"], z[f"{k}.gy"]
    assert_bit_equal(port_oracle.lga_forward(x, f, r), z[f"{k}.y"], "y")
    gx, gf = port_oracle.lga_backward(x, f, gy, r)
    assert_bit_equal(gx, z[f"{k}.gx"], "gx")
    assert_bit_equal(gf, z[f"{k}.gf"], "gf")
