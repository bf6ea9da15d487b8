"""CPU checks of the adaptive server optimizers that need no GPU: the binding table against include/fedserveropt.h,
the build's source lists, fso_step_plan against its restatement at the shapes where the launch changes, the rounding of
the hyper-parameters, the modes TorchServerOptimizer builds, the float32 restatement (tests/serveropt_fixtures.py)
against a float64 evaluation, and the fields of the measured profile."""
import argparse
import json
import os
import re

import numpy as np
import pytest

from fedscale_amd import _native_serveropt as ns
from fedscale_amd import buildinfo
from fedscale_amd import kernels_serveropt as kso
from tests import serveropt_fixtures as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- binding and build ------------------------------------------------------------------------------------------------
def test_binding_table_lists_exactly_the_headers_symbols_and_version():
    with open(os.path.join(ROOT, "include", "fedserveropt.h")) as f:
        hdr = f.read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(fso_\w+)\s*\(", body))
    assert declared == set(ns.SIGNATURES) == {"fso_abi_version", "fso_step", "fso_step_parts", "fso_step_plan"}
    assert int(re.search(r"#define FSO_ABI_VERSION (\d+)", hdr).group(1)) == ns.ABI_VERSION == 1
    assert int(re.search(r"#define FSO_PLAN_FIELDS (\d+)", hdr).group(1)) == ns.PLAN_FIELDS == 4
    assert re.search(r"#define FSO_NT_MIN_BYTES \(256LL << 20\)", hdr) and ns.NT_MIN_BYTES == sf.NT_MIN_BYTES == 256 << 20
    enums = dict(re.findall(r"\b(FSO_[A-Z_]+) = (\d+)", body))
    assert {k: int(v) for k, v in enums.items()} == {
        "FSO_ADAM": ns.ADAM, "FSO_ADAGRAD": ns.ADAGRAD, "FSO_AVGM": ns.AVGM, "FSO_INIT": ns.FSO_INIT,
        "FSO_NT_ON": ns.FSO_NT_ON, "FSO_NT_OFF": ns.FSO_NT_OFF}
    assert kso.RULES == {"adam": 0, "adagrad": 1, "avgm": 2} and tuple(kso.RULES) == sf.RULES
    lib = ns.load()
    assert lib.fso_abi_version() == ns.ABI_VERSION
    for name in ns.SIGNATURES:
        assert hasattr(lib, name)
    for fn, (_, args) in ns.SIGNATURES.items():  # the argument counts of the header's prototypes
        proto = re.search(r"\b%s\s*\(([^;]*)\);" % fn, body).group(1)
        n = 0 if proto.strip() == "void" else proto.count(",") + 1
        assert n == len(args), fn


def test_the_unit_and_header_are_in_the_build():
    assert "fedscale_amd/csrc/server_opt.hip" in buildinfo.SRCS and "include/fedserveropt.h" in buildinfo.HDRS


# ---- fso_step_plan ----------------------------------------------------------------------------------------------------
def _plan_sizes():
    out = [0, 1, 4, 5, 1023, 1024, 1025, sf.LAST_ONE_TRIP_P, sf.LAST_ONE_TRIP_P + 1]
    for rule in ("avgm", "adam"):  # 5 and 7 streams
        out += [sf.last_cached_P(rule), sf.last_cached_P(rule) + 1]
    return out + [25_000_000, 100_000_000]


@pytest.mark.parametrize("rule", sf.RULES)
def test_plan_equals_its_restatement(rule):
    for P in _plan_sizes():
        for init in (False, True):
            for nt in (None, True, False):
                assert kso.plan(rule, P, init=init, nt=nt) == sf.plan(rule, P, init=init, nt=nt), (rule, P, init, nt)


def test_plan_at_the_shapes_where_the_launch_changes():
    assert kso.plan("adam", 0) == dict(blocks=0, trips=0, nt=False, bytes=0)
    assert kso.plan("adam", 1) == dict(blocks=1, trips=1, nt=False, bytes=7 * 16)
    assert kso.plan("avgm", 4) == dict(blocks=1, trips=1, nt=False, bytes=5 * 16)
    assert kso.plan("avgm", 5, init=True) == dict(blocks=1, trips=1, nt=False, bytes=2 * 4 * 16)
    assert kso.plan("adagrad", 5, init=True)["bytes"] == 2 * 5 * 16
    P1 = sf.LAST_ONE_TRIP_P
    assert P1 == 8192 * 256 * 4
    assert kso.plan("adam", P1)["trips"] == 1 and kso.plan("adam", P1)["blocks"] == 8192
    assert kso.plan("adam", P1 + 1)["trips"] == 2 and kso.plan("adam", P1 + 1)["blocks"] == 8192
    assert kso.plan("adam", 4 * P1 + 1)["trips"] == 5
    for rule, streams in (("adam", 7), ("adagrad", 7), ("avgm", 5)):
        Pc = sf.last_cached_P(rule)
        assert Pc * 4 * streams <= 256 << 20 < (Pc + 4) * 4 * streams  # the threshold in bytes of the rule's streams
        assert not kso.plan(rule, Pc)["nt"] and kso.plan(rule, Pc + 1)["nt"]
        assert kso.plan(rule, Pc, nt=True)["nt"] and not kso.plan(rule, Pc + 1, nt=False)["nt"]
        assert kso.plan(rule, 5, nt=True)["nt"]  # the override reaches the non-temporal path at a small P
    assert sf.last_cached_P("avgm") > sf.last_cached_P("adam")  # fewer streams: a longer model still fits the cache


def test_plan_refuses_what_the_step_refuses():
    lib = ns.load()
    f = np.zeros(4, dtype=np.int64)
    for what, (rule, P, flags) in {"negative P": (0, -1, 0), "unknown rule": (3, 8, 0), "negative rule": (-1, 8, 0),
                                   "both NT flags": (0, 8, ns.FSO_NT_ON | ns.FSO_NT_OFF),
                                   "unknown flag": (0, 8, 8)}.items():
        assert lib.fso_step_plan(rule, P, flags, f.ctypes.data) == -1, what
        msg = lib.fa_last_error_string().decode()
        assert "fso_step_plan" in msg and "nothing was launched" in msg, (what, msg)
    assert lib.fso_step_plan(0, 8, 0, None) == -1 and "fields" in lib.fa_last_error_string().decode()
    assert not f.any()
    with pytest.raises(ValueError, match="rule"):
        kso.plan("yogi", 8)


# ---- hyper-parameters and modes ---------------------------------------------------------------------------------------
def test_fp32_hparams_rounding():
    from fedscale_amd.utils.optimizer.adaptive import FedAdagrad, FedAdam, FedAvgM

    o = FedAdam(eta=0.1, tau=1e-3, beta=0.9, beta2=0.99)
    h = o.fp32_hparams()
    assert set(h) == {"eta", "tau", "beta", "omb", "beta2", "omb2", "v0"}
    assert h == {k: float(v) for k, v in sf.hparams(0.1, 1e-3, 0.9, 0.99).items()}
    # 1 - beta is formed in double and rounded once; fp32(1) - fp32(beta) is another number
    assert h["omb"] == float(F32(1.0 - 0.9)) != float(F32(1.0) - F32(0.9))
    assert h["omb2"] == float(F32(1.0 - 0.99)) != float(F32(1.0) - F32(0.99))
    # v0 defaults to tau*tau in double, rounded once; fp32(tau)^2 in fp32 is another number
    assert h["v0"] == float(F32(1e-3 * 1e-3)) != float(F32(1e-3) * F32(1e-3))
    assert FedAdam(v0=0.5).fp32_hparams()["v0"] == 0.5 and FedAdagrad(tau=0.0).fp32_hparams()["v0"] == 0.0
    assert FedAvgM().eta == 1.0 and FedAdam().eta == FedAdagrad().eta == 1e-2
    for cls in (FedAdam, FedAdagrad, FedAvgM):
        o = cls()
        assert o.exposes_device_state is True and not o.initialized and o.m is None and o.m_t == [] and o.v_t == []
    from fedscale_amd.utils.optimizer.yogi import YoGi

    assert YoGi.exposes_device_state is True


def test_server_optimizer_builds_each_mode_from_bare_and_full_args():
    from fedscale_amd.cloud.aggregation.optimizers import STEP_MODES, TorchServerOptimizer
    from fedscale_amd.utils.optimizer.adaptive import MODES, FedAdagrad, FedAdam, FedAvgM

    assert MODES == {"fed-adam": FedAdam, "fed-adagrad": FedAdagrad, "fed-avgm": FedAvgM}
    assert set(STEP_MODES) == {"fed-yogi", "q-fedavg"} | set(MODES)
    for mode, cls in MODES.items():
        o = TorchServerOptimizer(mode, argparse.Namespace(), "cuda:0")
        c = o.gradient_controller
        assert type(c) is cls and o.mode == mode
        assert (c.eta, c.tau, c.beta, c.beta2, c.v0) == (1.0 if mode == "fed-avgm" else 1e-2, 1e-3, 0.9, 0.99, None)
        full = argparse.Namespace(server_eta=0.5, server_tau=1e-2, server_beta=0.8, server_beta2=0.95, server_v0=0.25)
        c = TorchServerOptimizer(mode, full, "cuda:0").gradient_controller
        assert (c.eta, c.tau, c.beta, c.beta2, c.v0) == (0.5, 1e-2, 0.8, 0.95, 0.25)
        s = TorchServerOptimizer(mode, full, "cuda:0").for_shard("cuda:1")
        assert s.mode == mode and type(s.gradient_controller) is cls and s.gradient_controller.eta == 0.5
    # the reference's modes are what they were
    assert not hasattr(TorchServerOptimizer(None, argparse.Namespace(), "cuda:0"), "gradient_controller")
    assert not hasattr(TorchServerOptimizer("fed-avg", argparse.Namespace(), "cuda:0"), "gradient_controller")


# ---- the restatement against float64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", sf.RULES)
def test_restatement_against_float64_on_well_conditioned_inputs(rule):
    """|g|, m and v in [1e-3, 1e3], m and g of one sign so that no sum cancels.  Every fp32 operation adds a relative
    error of at most u = 2^-24 to its result and, cancellation excluded, passes its operands' relative errors on
    (a square root halves its operand's).  Counting the roundings on the longest path to each result — inputs exact:
        m:    beta*m and omb*g (1 each, in parallel), their sum (1), after g = cur - last (1)           -> 3 u
        v:    g (1), g*g (doubles g's error: 2 + 1), omb2 * (1), beta2*v (1, parallel), the sum (1)     -> 5 u
        step: m (3) and den = sqrt(v) (5/2 + 1) + tau (1) meet in the quotient (3 + 4.5 + 1), eta * (1) -> 9.5 u
    The step is compared, not last + step: |last| may exceed the step by 1e6, and then the sum's own rounding of
    last is all that is left: out = fp32(last + step) adds at most u * |out| to the step's error.  The bounds below
    are those counts times 2^-24, the step's rounded up to a whole count (4 u for avgm's eta * m), and all of them
    times 1.001 for the second-order terms the counting drops."""
    u = 2.0 ** -24 * 1.001
    rng = np.random.default_rng(17)
    n = 4096
    mag = lambda: np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n))  # noqa: E731
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    last = (rng.standard_normal(n)).astype(F32)
    g = (sign * mag()).astype(F32)
    cur = (last + g).astype(F32)
    m = (sign * mag()).astype(F32)
    v = mag().astype(F32)
    hp = sf.hparams(eta=0.05, tau=1e-3, beta=0.9, beta2=0.99)
    g32 = (cur - last).astype(np.float64)
    keep = (np.abs(g32) >= 1e-3) & (np.sign(g32) == sign)  # cur = fp32(last + g) kept g's size and sign
    assert keep.sum() > n // 2
    m1, v1, out = sf.step(rule, cur, last, m, v, hp, False)
    M1, V1, OUT = sf.step64(rule, cur, last, m, v, hp, False)
    rel = lambda a, b: np.max(np.abs(a.astype(np.float64)[keep] - b[keep]) / np.abs(b[keep]))  # noqa: E731
    # both evaluations start from the same fp32 cur and last; the float64 difference cur - last is exact
    assert rel(m1, M1) <= 3 * u, rel(m1, M1)
    if rule != "avgm":
        assert rel(v1, V1) <= 5 * u, rel(v1, V1)
    lastd = last.astype(np.float64)
    step32 = out.astype(np.float64) - lastd
    step64 = OUT - lastd
    bound = (4 if rule == "avgm" else 10) * u * np.abs(step64) + u * np.abs(OUT)
    assert np.all(np.abs(step32 - step64)[keep] <= bound[keep])
    # the first step: m = 0 and v = v0
    m1, v1, out = sf.step(rule, cur, last, None, None, hp, True)
    M1, V1, OUT = sf.step64(rule, cur, last, None, None, hp, True)
    assert rel(m1, M1) <= 3 * u
    if rule != "avgm":
        assert rel(v1, V1) <= 5 * u


def test_avgm_with_beta_zero_and_eta_one_is_not_always_the_mean():
    hp = sf.hparams(eta=1.0, beta=0.0)
    last = np.asarray([1.0, 1e8, -3.0], dtype=F32)
    cur = np.asarray([1.0 + 2.0 ** -23, 1.0, 1e-8], dtype=F32)
    _, _, out = sf.step("avgm", cur, last, None, None, hp, True)
    assert sf.bits_equal(out, (last + (cur - last)).astype(F32))
    assert out[0] == cur[0] and out[1] != cur[1] and out[2] != cur[2]  # last + (mean - last), as documented


def test_bits_equal_treats_nans_by_class_and_zeros_by_sign():
    a = np.asarray([0.0, np.nan, 1.0], dtype=F32)
    b = a.copy()
    b.view(np.uint32)[1] = 0xFFC00001  # another NaN
    assert sf.bits_equal(a, b)
    b[0] = -0.0
    assert not sf.bits_equal(a, b) and "first at 0" in sf.first_difference(a, b)
    assert not sf.bits_equal(a, a[:2])


# ---- the profile ------------------------------------------------------------------------------------------------------
def test_measured_profile_has_its_fields():
    with open(os.path.join(ROOT, "profiles", "serveropt_measure.json")) as f:
        doc = json.load(f)
    assert isinstance(doc["device"], str) and doc["device"] and re.fullmatch(r"[0-9a-f]{16}", doc["build_id"]) and doc["build_defs"] == ""
    assert doc["calls_per_median"] >= 20
    assert doc["bytes_per_parameter"] == {"adam": 28, "adagrad": 28, "avgm": 20, "yogi": 28}
    assert set(doc["predictions"]) == {"adam", "adagrad", "avgm", "met_when"}
    assert [s["P"] for s in doc["steps"]] == [1_000_000, 25_000_000]
    for s in doc["steps"]:
        y = s["k_yogi_step"]
        assert 0 < y["ms_min"] <= y["ms_median"] <= y["ms_max"] and y["bytes"] == 28 * s["P"]
        for rule in sf.RULES:
            r = s[rule]
            for path in ("nt_on", "nt_off"):
                e = r[path]
                assert 0 < e["ms_min"] <= e["ms_median"] <= e["ms_max"] and e["TBps"] > 0
                assert e["bytes"] == doc["bytes_per_parameter"][rule] * s["P"]
            assert r["policy_nt"] == sf.plan(rule, s["P"])["nt"]
            assert isinstance(r["policy_takes_the_faster_path"], bool)
            assert r["yogi_spread_ms"] == [y["ms_min"], y["ms_max"]]
            chosen = r["nt_on" if r["policy_nt"] else "nt_off"]["ms_median"]
            implied = chosen * 28 / doc["bytes_per_parameter"][rule]
            assert abs(r["implied_yogi_ms"] - implied) < 1e-3
            assert r["prediction"] == ("met" if y["ms_min"] <= r["implied_yogi_ms"] <= y["ms_max"] else "missed")
    rd = doc["round"]
    assert (rd["K"], rd["P"]) == (1000, 25_000_000) and rd["reps"] >= 3
    for k in ("fed_yogi_round", "fed_adam_round"):
        assert 0 < rd[k]["ms_min"] <= rd[k]["ms_median"] <= rd[k]["ms_max"]
    a, y = rd["fed_adam_round"], rd["fed_yogi_round"]
    assert rd["prediction"] == ("met" if y["ms_min"] <= a["ms_median"] <= y["ms_max"] else "missed")
