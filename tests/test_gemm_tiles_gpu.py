"""GPU: every tile of the MFMA GEMM through every epilogue (csrc/gemm_f32.hip, csrc/mfma_tile.h) at small shapes - the
128 x 128, 256 x 128, 128 x 96 and 128 x 32 tiles are otherwise reached by production-size cases only."""
import pytest
import torch

from tests import _gemm_tile_cases as tc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", tc.CASES, ids=[c.id for c in tc.CASES])
def test_tile_and_epilogue_match_fp64(case, dfx_env):
    from dfx import ops
    dfx_env("DFX_GEMM_NO_ROWS", "1")
    dfx_env("DFX_GEMM_TILE", case.env)
    t = tc.inputs(case)
    want = tc.reference(case, t)
    # Every element is compared with the reference below, which is what catches one the kernel does not write: stale memory
    # does not match.  The result is allocated by the call, so as a best effort on top (the allocator is free to hand out
    # another block) NaNs are left in a block of its size, freed just before: a stale value equal to an earlier case's fails too.
    poison = torch.full(want.shape, float("nan"), device="cuda")
    del poison
    ops.profile_start()
    got = tc.run(case, t)
    tiles = [tb for (_, _, ta, tb) in ops.profile_stop() if ta in (-1, -2)]
    # (one launch; a K-block-major x goes through in row ranges of 256, whose last 44 rows the rule gives to the 64 x 128 tile)
    assert tiles[:1] == [case.expect] and (case.env is None or set(tiles) == {case.expect}), \
        f"the case must run on the tile it is meant for, not {tiles}"
    assert len(tiles) == (2 if case.variant == "xblocked_res" else 1)
    assert got.shape == want.shape
    err = (got.double() - want).abs().max().item()          # the whole tensor: masked rows are zeros in both
    print(f"{case.id}: max error {err:.3e}, bound {tc.tolerance(case):.3e}")
    assert err < tc.tolerance(case)
