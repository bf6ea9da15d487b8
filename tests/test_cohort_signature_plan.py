"""CPU checks of the Auxo signature path: ``signature_plan`` maps the reference's concatenate-and-slice
(examples/auxo/client_metadata.py:13-16) onto the flat layout exactly, include/fedcohort.h and its binding table
agree, and the entry points validate their arguments before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fedscale_amd.bucket import BucketLayout
from fedscale_amd.cohort_signature import signature_plan
from tests.cohort_sig_fixtures import FIXTURES, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_tail(layout: BucketLayout):
    """The concatenation indices the reference keeps: its own two lines on per-tensor arrays that hold their
    position in the concatenation (int64 entries make it float64, as in the reference)."""
    tensors, c = [], 0
    for e in layout.entries:
        dt = np.float32 if e.kind == "f" else np.int64
        tensors.append(np.arange(c, c + e.numel, dtype=np.float64).astype(dt).reshape(e.shape))
        c += e.numel
    gradient = np.concatenate([v.flatten() for v in tensors])
    val_len = len(gradient) // 10
    return gradient[-val_len:], c


def _check_plan(layout: BucketLayout):
    plan = signature_plan(layout)
    want, N = _reference_tail(layout)
    assert plan.N == N and plan.D == len(want)
    # the device buffers, holding every element's concatenation index
    f32 = np.zeros(max(1, layout.P_full), dtype=np.float32)
    side = np.zeros(max(1, layout.Q), dtype=np.int64)
    c = 0
    for e in layout.entries:
        dst = f32 if e.kind == "f" else side
        dst[e.offset:e.offset + e.numel] = np.arange(c, c + e.numel)
        c += e.numel
    np.testing.assert_array_equal(plan.gather(f32, side), want.astype(np.float64))
    # segments: inside the buffers, disjoint, and together with the int64 elements exactly [0, D)
    cover = np.zeros(plan.D, dtype=np.int64)
    for src, dst, n in plan.segs.tolist():
        assert n > 0 and 0 <= src and src + n <= layout.P_full and 0 <= dst and dst + n <= plan.D
        cover[dst:dst + n] += 1
    for q, dst in plan.isegs.tolist():
        assert 0 <= q < layout.Q and 0 <= dst < plan.D
        cover[dst] += 1
    assert (cover == 1).all()
    assert len(plan.segs) <= len(plan.isegs) + 1
    assert plan.ldd >= plan.D and plan.ldd % 64 == 0
    return plan


@pytest.mark.parametrize("name", FIXTURES)
def test_plan_matches_the_reference_slice_on_fixture_layouts(name):
    fx = load(name)
    layout = BucketLayout.from_state_dict(fx.module().state_dict())
    plan = _check_plan(layout)
    assert plan.D == fx.expected("sig").shape[1]
    if name == "auxo_sig_tiny_k5":
        assert plan.N == 2 and plan.D == 2  # N < 10: gradient[-0:] is the whole vector
    if name == "auxo_sig_mixed_k9":
        assert len(plan.isegs) == 1 and layout.Q == 2  # one of the two int64 buffers lies inside the tail
        assert len(plan.segs) == 2 and any(s % 4 for s, _, _ in plan.segs.tolist())  # a misaligned start
    if name == "auxo_sig_femnist_cnn_k10":
        assert layout.P_full == 24492 and plan.D == 2449


def test_plan_matches_the_reference_slice_on_random_layouts():
    rng = np.random.default_rng(2024)
    seen_small = seen_int_tail = 0
    for it in range(300):
        T = int(rng.integers(1, 13))
        N = int(rng.integers(1, 5001)) if it % 5 else int(rng.integers(1, 12))
        cuts = np.sort(rng.integers(0, N + 1, size=T - 1)) if T > 1 else np.zeros(0, dtype=np.int64)
        sizes = np.diff(np.concatenate([[0], cuts, [N]])).astype(int)
        names, shapes, dtypes = [], [], []
        for i, n in enumerate(sizes.tolist()):
            as_int = rng.random() < 0.3
            if as_int and n > 3:
                n_int = int(rng.integers(1, 4))  # int64 buffers are small: the rest of the run stays fp32
                names += [f"t{i}", f"t{i}.count"]
                shapes += [(n - n_int,), (n_int,) if n_int > 1 else ()]
                dtypes += [torch.float32, torch.int64]
            else:
                names.append(f"t{i}")
                shapes.append((n,) if n != 1 or rng.random() < 0.5 else ())
                dtypes.append(torch.int64 if as_int else torch.float32)
        layout = BucketLayout(names, shapes, dtypes)
        assert layout.P_full + layout.Q == N
        plan = _check_plan(layout)
        seen_small += N < 10
        seen_int_tail += len(plan.isegs) > 0
    assert seen_small >= 20 and seen_int_tail >= 20


def test_sharded_layout_is_refused():
    layout = BucketLayout(["w"], [(1000,)], [torch.float32], rank=1, world=2)
    with pytest.raises(NotImplementedError, match="parameter-sharded"):
        signature_plan(layout)


def _header_functions():
    src = open(os.path.join(ROOT, "include", "fedcohort.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fc_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_symbol_of_fedcohort_h():
    from fedscale_amd import _native, _native_cohort, buildinfo

    lib = ctypes.CDLL(_native.LIB_PATH)
    names = _header_functions()
    assert len(names) >= 7
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/fedcohort.h but not exported"
    assert sorted(_native_cohort.SIGNATURES) == names, "ctypes binding out of sync with include/fedcohort.h"
    assert not set(_native_cohort.SIGNATURES) & set(_native.SIGNATURES)
    assert _native_cohort.load().fc_abi_version() == _native_cohort.ABI_VERSION
    assert _native.load().fa_abi_version() == 5  # the new header leaves FA_ABI_VERSION alone
    # the build id covers the new translation unit and header
    assert "fedscale_amd/csrc/cohort_sig.hip" in buildinfo.SRCS and "include/fedcohort.h" in buildinfo.HDRS


def test_argument_errors_without_gpu():
    """Validation precedes any HIP call (fake device addresses are never dereferenced)."""
    from fedscale_amd import _native_cohort as nc
    from fedscale_amd._native import FedAggError

    lib = nc.load()
    seg = np.asarray([[60, 0, 8]], dtype=np.int64)  # src + len = 68 > ld = 64
    with pytest.raises(FedAggError, match="segment 0"):
        nc.call("fc_signature", 256, 64, 2, 512, None, 1, None, seg.ctypes.data, 1, None, 0, 1024, 64, None)
    seg = np.asarray([[0, 60, 8]], dtype=np.int64)  # dst + len = 68 > ldd = 64
    with pytest.raises(FedAggError, match="segment 0"):
        nc.call("fc_signature", 256, 64, 2, 512, None, 1, None, seg.ctypes.data, 1, None, 0, 1024, 64, None)
    iseg = np.asarray([[3, 0]], dtype=np.int64)  # side index 3 of a 3-entry table
    with pytest.raises(FedAggError, match="int64 element 0"):
        nc.call("fc_signature", None, 64, 2, None, 256, 3, 512, None, 0, iseg.ctypes.data, 1, 1024, 64, None)
    with pytest.raises(FedAggError, match="at most 4096"):
        nc.call("fc_gram", 256, 64, 4097, 64, 512, 1024, None)
    assert lib.fc_gram_workspace_bytes(4097, 64) == 0
    with pytest.raises(FedAggError, match="bad arguments"):
        nc.call("fc_center", 256, 8, 4, 16, 512, 1024, 2048, 4096, None)  # ldd < D
    with pytest.raises(FedAggError, match="alias"):
        nc.call("fc_center", 256, 16, 4, 16, 512, 256, 2048, 4096, None)
    with pytest.raises(FedAggError, match="bad arguments"):
        nc.call("fc_normalize", 256, 16, 0, 16, 512, 1024, None)
    # workspace sizes: per-wave fp64 partial rows + the 32 segment rows; [nsplit][K][K] fp32
    assert lib.fc_center_workspace_bytes(10, 2449) == (5 + 32) * 10 * 8
    assert lib.fc_gram_workspace_bytes(5, 7) == 5 * 5 * 4
    assert lib.fc_gram_workspace_bytes(1000, 1119126) % (1000 * 1000 * 4) == 0


def test_sharded_adapter_refuses_signatures():
    """A model sharded over several parts has no whole-model tail on any one device: begin_round(signatures=True)
    raises NotImplementedError before it touches a device (and takes the keyword at all)."""
    from fedscale_amd.cloud.internal.sharded_model_adapter import ShardedModelAdapter

    ad = object.__new__(ShardedModelAdapter)
    ad.parts = [None, None]
    with pytest.raises(NotImplementedError, match="cohort signatures"):
        ad.begin_round(3, "fedavg", signatures=True)


def test_cohort_mixin_with_the_switch_off_needs_nothing_new_of_a_round():
    """With device_cohort_signatures off the mixin asks a round for nothing but add(): rounds of adapters that
    know no signatures (ShardedModelAdapter's ShardedRound has no ``sig_plan``) work as before."""
    from fedscale_amd.cloud.aggregation.aggregator import DeviceCohortAggregator
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    class PlainRound:  # as ShardedRound: no sig_plan attribute
        def __init__(self):
            self.added = []

        def add(self, update):
            self.added.append(update)

    class Adapter(TorchModelAdapter):
        def __init__(self):
            self.rounds, self.applied = [], []

        def begin_round(self, K, policy, capacity=None, keep_mean=True):  # the signature before this feature
            self.rounds.append(PlainRound())
            return self.rounds[-1]

        def apply_round(self, rnd, denom32, denom64, client_training_results=None, keep_mean=True):
            self.applied.append((rnd, denom32, denom64))

        def round_mean_weights(self):
            return ["mean"]

    w = Adapter()
    agg = DeviceCohortAggregator([w], [3])
    for k in range(3):
        agg.on_result({"client_id": k, "update_weight": [k]}, 0)
    assert len(w.rounds) == 1 and w.rounds[0].added == [[0], [1], [2]]
    assert w.applied == [(w.rounds[0], 3.0, 3.0)] and agg.model_weights[0] == ["mean"]
    assert not hasattr(agg, "cohort_signatures") and not hasattr(agg, "_cohort_round_clients")
