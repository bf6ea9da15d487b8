"""Host-only checks of the majority-vote path: the encoder's bytes, ``VoteSpec``, the launch plan and the build
lists."""
import pickle

import numpy as np
import pytest
import torch


@pytest.mark.parametrize("P", [1, 9, 257])
def test_compress_vote_is_packbits_of_the_sign_bits(P):
    from fedscale_amd.cloud.execution.vote_upload import VOTE_BITS_KEY, compress_vote

    rng = np.random.default_rng(P)
    L = rng.standard_normal(P).astype(np.float32)
    x = (L + rng.standard_normal(P).astype(np.float32)).astype(np.float32)
    x[0] = L[0] = np.float32(-0.0)  # -0.0 - -0.0 = +0.0: votes up
    up = compress_vote({"w": torch.from_numpy(x), "steps": np.asarray(3)}, [L, np.asarray(0)])
    assert list(up) == ["steps", VOTE_BITS_KEY] and up[VOTE_BITS_KEY].dtype == np.uint8
    assert np.array_equal(up[VOTE_BITS_KEY], np.packbits(np.signbit(x - L), bitorder="little"))
    assert up[VOTE_BITS_KEY].size == (P + 7) // 8 and up[VOTE_BITS_KEY][0] & 1 == 0


def test_vote_spec_validation():
    from fedscale_amd.cloud.execution.vote_upload import VoteSpec

    assert VoteSpec.of(0.01) == VoteSpec(0.01, "majority") and VoteSpec(0.5, "mean").mode == "mean"
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-60):
        with pytest.raises(ValueError, match="upload_vote"):
            VoteSpec(bad)
    with pytest.raises(ValueError, match="mode"):
        VoteSpec(0.1, "median")
    with pytest.raises(TypeError):
        VoteSpec("0.1")


@pytest.mark.parametrize("cus", [8, 256, 304])
@pytest.mark.parametrize("P", [1, 2049, 24492, 1_000_003, 25_000_000])
def test_count_votes_plan_covers_every_strip_once(cus, P):
    from fedscale_amd.kernels_vote import count_votes_plan

    strips = ((P + 31) // 32 + 63) // 64
    for n in (1, 33, 1000, 65535):
        plan = count_votes_plan(cus, n, P)
        assert plan == count_votes_plan(cus, n, P)  # a function of (cus, n, P) alone
        col = 0
        for l in plan:
            assert l["col0"] == col and l["grid"] <= l["tiles"] and l["S"] == plan[0]["S"] >= 1
            col += l["tiles"] * 4 * l["V"] * 2048
        assert (strips - 1) * 2048 < col - 0 and col < (strips + 4 * plan[-1]["V"]) * 2048
        S = plan[0]["S"]
        assert S == 1 or (sum(l["tiles"] for l in plan) < cus and n // S >= 256)  # a slice is at least 256 rows
        assert S > 1 or not (P == 2049 and n >= 1000), "one tile on any card: 1000 rows and more are split"


def test_buildinfo_lists_the_new_unit():
    from fedscale_amd import buildinfo

    assert "fedscale_amd/csrc/vote_reduce.hip" in buildinfo.SRCS and "include/fedvote.h" in buildinfo.HDRS


def test_the_adapter_pickles_with_its_spec():
    from fedscale_amd.cloud.execution.vote_upload import VoteSpec
    from fedscale_amd.cloud.internal import torch_model_adapter as tma

    spec = VoteSpec(0.25, "mean")
    assert pickle.loads(pickle.dumps(spec)) == spec and tma.TorchModelAdapter.upload_vote is None
    a = object.__new__(tma.TorchModelAdapter)
    a.model, a.optimizer, a.upload_vote = torch.nn.Linear(2, 2), None, spec
    a.get_model = lambda: a.model
    fn, args = a.__reduce__()
    assert fn is tma._rebuild_with_upload_vote and args[0] is tma.TorchModelAdapter and args[3] == spec
