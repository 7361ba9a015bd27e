"""The limits of the one-shape library, stated twice and held to each other: csrc/rr_sim.hpp's constexpr shape_lanes (what Cfg asserts,
so what hipcc accepts) as the host emulations export it -- the default and the parity build -- and roborugby_amd.build.shape_lanes
(what refuses a shape before any compiler runs)."""
import itertools
import time

import pytest

import emu_lib as el


@pytest.mark.parametrize("exact", [False, True])
def test_shape_lanes_agrees_with_the_kernel_sources_on_the_whole_grid(exact):
    from roborugby_amd import build
    kernel = el.lib(exact).emu_shape_lanes
    accepted = {}
    for nrh, nrg, nbp, nbn in itertools.product(range(10), range(10), range(13), range(13)):
        want = kernel(nrh, nrg, nbp, nbn)
        try:
            got = build.shape_lanes(nrh, nrg, nbp, nbn, exact=exact)
        except ValueError as exc:
            assert len(str(exc)) > 20, (nrh, nrg, nbp, nbn)  # it names the limit
            got = 0
        assert got == want, ((nrh, nrg, nbp, nbn), exact, got, want)
        if want:
            accepted[(nrh, nrg, nbp, nbn)] = want
    # the grid reaches past every limit, and the accepted part holds every lane width and the pinned limit shapes
    assert set(accepted.values()) == {2, 4, 8, 16}
    assert accepted[(1, 1, 4, 7)] == 16 and accepted[(4, 4, 2, 2)] == 8 and accepted[(2, 2, 3, 3)] == 8 and accepted[(2, 1, 2, 3)] == 8
    assert ((1, 0, 3, 0) in accepted) == (not exact) and ((1, 0, 2, 0) in accepted) == (not exact) and (1, 0, 1, 0) in accepted
    assert max(a + b for a, b, _, _ in accepted) == 8 and max(c + d for _, _, c, d in accepted) == 11
    assert max((a + b) * (c + d) for a, b, c, d in accepted) == 32
    assert all(c * (1 + a + b) <= 6 * (a + b) for a, b, c, _ in accepted)


def test_shapes_that_cannot_build_are_refused_before_any_compiler_runs():
    """(2, 0, 6, 5) overflows the reward scratch, the parity build has no one-robot carry chain for two balls: a ValueError at once, from
    shape_lanes and from the paths that would otherwise start hipcc."""
    from roborugby_amd import _lib, build
    t0 = time.perf_counter()
    with pytest.raises(ValueError, match="reward scratch"):
        build.shape_lanes(2, 0, 6, 5)
    with pytest.raises(ValueError, match="parity build"):
        build.shape_lanes(1, 0, 2, 0, exact=True)
    assert build.shape_lanes(1, 0, 2, 0) == 2
    for counts, exact in (((2, 0, 6, 5), False), ((1, 0, 4, 0), False), ((1, 0, 2, 0), True)):
        with pytest.raises(ValueError):
            build.build_shape_library(*counts, exact=exact)
        with pytest.raises(ValueError):
            _lib.load_shape(counts, exact=exact)
    assert time.perf_counter() - t0 < 1.0
