"""SGA held to a float64 statement of its definition (tests/sga_ref64.py, written from SURVEY Appendix A.1 / A.2): the reference
against calculus, the C oracle (and the reference's own kernel bodies where oracle/_ref is built) against the reference, and
the emulator build of the library against the reference -- equality on the exact *select* family, a per-element first-order
rounding bound times 2 on continuous inputs (tests/sga_ref64_cases.py).  The same cases run on the gfx950 build in
tests/test_gpu_sga_ref64.py."""
import numpy as np
import pytest

import parity_cases as pc
import sga_ref64 as r64
import sga_ref64_cases as sc
import value_cases as vc

DEV = pc.NumpyDev()
TINY, TINY_SEED = (1, 1, 4, 3, 4), 0                     # tie-free: every selection gap >= 1e-3 (asserted)
FIRST = [np.s_[:, :, :, 0, :], np.s_[:, :, :, -1, :], np.s_[:, :, :, :, 0], np.s_[:, :, :, :, -1]]      # first scan position of each direction
SELECT_SHAPES = list(dict.fromkeys(vc.SGA_DEFAULT_SHAPES + vc.SGA_TILED_SHAPES + sc.FORCED_SHAPES))
TEETH_SHAPE = (2, 1, 20, 9, 20)


@pytest.fixture(scope="module")
def sim():
    from sim_util import sim_api
    return sim_api()


@pytest.fixture(scope="module", params=["port", "reference"])
def oracle(request):
    from oracle import oracle as om
    if not om.have(request.param) and request.param == "reference":
        pytest.skip("oracle/_ref is not built")
    return om.Oracle(request.param)


# ---- (a) the reference against itself and against calculus ------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    x, gs, go = pc.sga_inputs(TINY, TINY_SEED)
    fwd = r64.forward(x, *gs)
    assert min(r64.selection_gaps(fwd)) >= 1e-3, r64.selection_gaps(fwd)
    return x.astype(np.float64), [g.astype(np.float64) for g in gs], go.astype(np.float64), fwd


def test_true_backward_is_the_gradient_of_forward(tiny):
    """central differences of sum(out * go) in float64, h = 1e-6, in every element of x and of the four guidances.  The map
    is piecewise bilinear and no selection is within 1e-3 of changing, so the difference quotient is exact up to rounding
    (eps / h ~ 1e-10 on O(1) values): 1e-7 absolute."""
    x, gs, go, fwd = tiny
    true = r64.true_backward(x, gs, go, fwd)
    args = [x] + gs
    h = 1e-6

    def f():
        return float((r64.forward(*args)["out"] * go).sum())

    worst = 0.0
    for a, key in zip(args, sc.GRADS):
        fd = np.empty_like(a)
        for i in np.ndindex(a.shape):
            keep = a[i]
            a[i] = keep + h
            up = f()
            a[i] = keep - h
            fd[i] = (up - f()) / (2 * h)
            a[i] = keep
        worst = max(worst, float(np.abs(fd - true[key]).max()))
        assert np.abs(fd - true[key]).max() <= 1e-7, (key, float(np.abs(fd - true[key]).max()))
        assert np.abs(true[key]).max() > 0.1, key
    print("largest |finite difference - true_backward|:", worst)


def test_backward_leaves_out_the_first_position_terms_and_nothing_else(tiny):
    """SURVEY F4, stated: at the first scan position p = 0 of a direction all five taps read x[0][d], so the true gradient has
        gradX[0][d] = G (w0 + w1 + w2 + w3 + w4),   gw_t[0] = sum_d G x   (t = 0..4);
    the reference's backward (A.2) has
        gradX[0][d] = G w0 + [d == 0] G w2 + [d == D-1] G w3,   gw0[0] = sum_d G x,   gw1..gw4[0] = 0.
    The missing terms are therefore  G (w1 + w2 + w3 + w4) - [d == 0] G w2 - [d == D-1] G w3  in gradX and  sum_d G x  in each
    of gw1..gw4.  Each direction's share of gradX and its guidance gradient differ by exactly these at p = 0 and agree to
    1e-12 everywhere else; the adjoint volumes are the same.  Not vacuous: in every direction each of the five missing terms
    exceeds 1e-3 (at most of the first-position elements: an adjoint column that no later element feeds is exactly 0)."""
    x, gs, go, fwd = tiny
    ref, true = r64.backward(x, gs, go, fwd), r64.true_backward(x, gs, go, fwd)
    total = np.zeros_like(x)
    for d in range(4):
        assert np.array_equal(ref[f"G{d}"], true[f"G{d}"])
        G0, w, x0 = ref[f"G{d}"][FIRST[d]], gs[d][FIRST[d]], x[FIRST[d]]              # [N,C,D,O], [N,C,5,O], [N,C,D,O]
        miss_x = G0 * w[:, :, 1:].sum(2, keepdims=True)
        miss_x[:, :, 0] -= G0[:, :, 0] * w[:, :, 2]
        miss_x[:, :, -1] -= G0[:, :, -1] * w[:, :, 3]
        miss_w = (G0 * x0).sum(2)                                                     # [N,C,O]
        for name, term in (("gradX", miss_x), ("gw", miss_w)):
            assert np.abs(term).max() > 1e-3 and (np.abs(term) > 1e-3).mean() >= 0.5, (d, name, np.abs(term))
        want_x = np.zeros_like(x)
        want_x[FIRST[d]] = miss_x
        assert np.abs(true[f"gx_dir{d}"] - ref[f"gx_dir{d}"] - want_x).max() <= 1e-12, d
        want_w = np.zeros_like(gs[d])
        want_w[FIRST[d]][:, :, 1:] = miss_w[:, :, None]
        assert np.abs(true[f"gw{d}"] - ref[f"gw{d}"] - want_w).max() <= 1e-12, d
        assert not ref[f"gw{d}"][FIRST[d]][:, :, 1:].any()
        total += want_x
    assert np.abs(true["gx"] - ref["gx"] - total).max() <= 1e-12
    interior = (true["gx"] - ref["gx"])[:, :, :, 1:-1, 1:-1]
    assert interior.size and np.abs(interior).max() <= 1e-12


def test_scan_is_forward_of_one_direction(tiny):
    x, gs, go, fwd = tiny
    for d in range(4):
        assert np.array_equal(r64.scan(x, gs[d], d), fwd[f"A{d}"])
    assert np.array_equal(fwd["tmp"], fwd["A3"]) and np.array_equal(fwd["kp"], np.stack([np.argmax(fwd[f"A{d}"], 2) for d in range(4)]))


# ---- (b) the oracle is the definition -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SELECT_SHAPES)
def test_oracle_equals_the_definition_on_select(oracle, shape):
    """ties included: volumes, out, mask, A_left, first arg-max and all five (integer) gradients, every bit"""
    x, gs, go, ref, want = sc.select_case(shape)
    got = sc.oracle_results(oracle, x, gs, go)
    sc.assert_selections_equal(got, ref, "select")
    sc.assert_equal(got, want, sc.FWD + sc.GRADS, "select")


@pytest.mark.parametrize("shape", sc.ALL_SHAPES)
def test_oracle_within_the_bound_on_randn(oracle, shape):
    x, gs, go, ref = sc.randn_case(shape)                    # (asserts that no selection can differ)
    got = sc.oracle_results(oracle, x, gs, go)
    sc.assert_selections_equal(got, ref, "randn")
    q = sc.assert_within_bound(got, ref, sc.FWD + sc.GRADS, ("randn", shape))
    print("oracle", oracle.kind, "randn", shape, "error / bound:", sc.fmt(q))


@pytest.mark.parametrize("shape", SELECT_SHAPES)
def test_oracle_gradients_within_the_bound_on_sparse(oracle, shape):
    """exact ties and inexact values: the selections are the oracle's own; with those, its volumes and its gradients are
    within the bound of float64"""
    x, gs, go, got, ref = sc.sparse_case(oracle, shape)
    q = sc.assert_within_bound(got, ref, sc.FWD + sc.GRADS, ("sparse", shape))
    print("oracle", oracle.kind, "sparse", shape, "error / bound:", sc.fmt(q))


# ---- (d) the comparison has teeth ---------------------------------------------------------------------------------------------
def _with(ref, mutant):
    return {**ref, **{k: mutant[k] for k in sc.GRADS}}


@pytest.mark.parametrize("drop", r64.DROPS)
def test_comparison_rejects_a_wrong_reference(port_oracle, drop):
    """one term of the backward wrong in the reference (sga_ref64.mutated): the comparisons of (b) fail.  On randn the bound
    decides, on *select* equality.  (`last_argmax` on randn: stable() rules every tie out, so first and last arg-max are the
    same element and the mutant is the reference itself -- asserted; only *select*, where half the pixels tie, can tell.)"""
    x, gs, go, ref = sc.randn_case(TEETH_SHAPE)
    got = sc.oracle_results(port_oracle, x, gs, go)
    sc.assert_within_bound(got, ref, sc.GRADS)
    wrong = _with(ref, r64.mutated(x, gs, go, ref, drop))
    if drop == "last_argmax":
        sc.assert_equal(wrong, ref, sc.GRADS)
    else:
        with pytest.raises(AssertionError):
            sc.assert_within_bound(got, wrong, sc.GRADS)
    x, gs, go, ref, want = sc.select_case(TEETH_SHAPE)
    got = sc.oracle_results(port_oracle, x, gs, go)
    sc.assert_equal(got, want, sc.GRADS)
    wrong = r64.mutated(x, gs, go, ref, drop)
    with pytest.raises(AssertionError):
        sc.assert_equal(got, wrong, sc.GRADS)


# ---- (c) the emulator build of the library ------------------------------------------------------------------------------------
def _emulator_per_dir(shape):
    return shape[2] < 100                                    # (the cross-check of the entry points triples the emulator's time)


@pytest.mark.parametrize("shape", vc.SGA_DEFAULT_SHAPES)
def test_sim_default_dispatch(sim, port_oracle, shape):
    sc.run_select(sim, DEV, shape)
    print("emulator randn", shape, "error / bound:", sc.fmt(sc.run_randn(sim, DEV, port_oracle, shape)))


@pytest.mark.parametrize("tiled", [0, 1])
@pytest.mark.parametrize("shape", vc.SGA_TILED_SHAPES)
def test_sim_tiled_workspace(sim, port_oracle, shape, tiled):
    with vc.option(sim, "GANET_SGA_TILED", tiled):
        assert sim.query("ganet_sga_workspace_layout", *shape) == tiled
        sc.run_select(sim, DEV, shape, seed=vc.seed_of(shape, 1 + tiled))
        print("emulator randn", shape, "tiled", tiled, "error / bound:", sc.fmt(sc.run_randn(sim, DEV, port_oracle, shape)))


@pytest.mark.parametrize("opt,value,restore,shapes", vc.SGA_FORCED, ids=[o[0] for o in vc.SGA_FORCED])
def test_sim_forced_kernel_families(sim, port_oracle, opt, value, restore, shapes):
    with vc.option(sim, opt, value, restore):
        for shape in shapes:
            sc.run_select(sim, DEV, shape, per_dir=_emulator_per_dir(shape))
            print("emulator randn", opt, value, shape, "error / bound:", sc.fmt(sc.run_randn(sim, DEV, port_oracle, shape)))


@pytest.mark.parametrize("shape", [vc.SGA_SEGMENT_FALLBACK_SHAPE, sc.WIDE_SCAN_DEEP_SHAPE], ids=["segment_fallback", "wide_scan_D300"])
def test_sim_deep_volumes(sim, port_oracle, shape):
    """D in (208, 272]: the 16-lane segment kernels; D > 272: the whole wavefront on one scanline"""
    sc.run_select(sim, DEV, shape, per_dir=False)
    print("emulator randn", shape, "error / bound:", sc.fmt(sc.run_randn(sim, DEV, port_oracle, shape)))


@pytest.mark.parametrize("shape", vc.SGA_COMPAT_SHAPES)
def test_sim_reference_buffer_contract(sim, shape):
    x, gs, go, ref, want = sc.select_case(shape, seed=vc.seed_of(shape, 5))
    pc.check_sga_compat(sim, DEV, x, gs, go, want)


@pytest.mark.parametrize("with_bn", [False, True])
@pytest.mark.parametrize("shape", vc.SGA_INFER_SHAPES)
def test_sim_forward_infer(sim, shape, with_bn):
    sc.run_select_infer(sim, DEV, shape, with_bn)
