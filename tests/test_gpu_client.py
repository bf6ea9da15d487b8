"""Client-side element-wise handlers on the GPU through the C ABI (include/fedclient.h).

* FedProx (fa_prox_update, ClientOptimizer.update_client_weight): bit-exact against the real reference's
  outputs (tests/golden/client_prox_*) and against the oracle on multi-launch tensor lists.
* Local DP (fa_dp_clip_coef + fa_dp_apply, privatize_update / clip_grad_norm_): against the reference's
  outputs (tests/golden/client_dp_*).  Tolerances, written here: the total norm within rtol 1e-6 (fp64 vs
  the reference's fp32 accumulation); recovered parameters within rtol 1e-6 of the reference when it
  clips and bit-exact when it does not; the device's noise is exactly fp32(z * sigma) with z its own
  counter-based N(0,1) stream, whose moments are checked statistically.
"""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests.golden_io import ClientScenario, scenario_names

pytestmark = pytest.mark.gpu


class NamedStateModule(torch.nn.Module):
    """Rebuild a module whose state_dict has exactly the given (dotted) names, order and param/buffer roles."""

    def __init__(self, names, tensors, is_param):
        super().__init__()
        for n, t, isp in zip(names, tensors, is_param):
            mod = self
            *path, leaf = n.split(".")
            for part in path:
                if not hasattr(mod, part):
                    mod.add_module(part, torch.nn.Module())
                mod = getattr(mod, part)
            t = torch.as_tensor(np.array(t))
            if isp:
                mod.register_parameter(leaf, torch.nn.Parameter(t, requires_grad=False))
            else:
                mod.register_buffer(leaf, t)


@pytest.mark.parametrize("name", [n for n in scenario_names("client") if "_prox_" in n])
def test_fedprox_matches_reference_fixture(gpu_device, name):
    import argparse

    from fedscale_amd.cloud.execution.optimizers import ClientOptimizer

    sc = ClientScenario(name)
    T = len(sc.meta["shapes"])
    glob = [torch.from_numpy(a).to(gpu_device) for a in sc.list("global", T)]
    conf = argparse.Namespace(gradient_policy="fed-prox", learning_rate=sc.meta["lr"], proxy_mu=sc.meta["mu"])
    opt = ClientOptimizer()
    for s in range(sc.meta["steps"]):
        model = NamedStateModule([f"p{i}" for i in range(T)], sc.list(f"in/{s}", T), [True] * T).to(gpu_device)
        opt.update_client_weight(conf, model, glob)
        for p, want in zip(model.parameters(), sc.list(f"out/{s}", T)):
            got = p.data.cpu().numpy()
            assert got.dtype == want.dtype and np.array_equal(got, want)


def _ragged_list(rng, T, device):
    sizes = [0, 1, 3, 4, 5, 4095, 4096, 4097, 12289] + list(rng.integers(1, 20000, size=T - 9))
    base = torch.from_numpy(rng.normal(0, 0.1, size=sum(sizes) + 3 * T).astype(np.float32)).to(device)
    ts, o = [], 0
    for i, n in enumerate(sizes):
        o += i % 3  # some views start off the 16-byte grid (scalar path)
        ts.append(base[o:o + n])
        o += n
    return ts


def test_fedprox_multi_launch_bit_exact(gpu_device):
    """130 ragged, partly unaligned tensors (three launch groups) against the oracle."""
    from fedscale_amd import kernels as kx
    from oracle.cpu_reference import fedprox_update

    rng = np.random.default_rng(5)
    params = _ragged_list(rng, 130, gpu_device)
    glob = [torch.from_numpy(rng.normal(0, 0.1, size=p.numel()).astype(np.float32)).to(gpu_device) for p in params]
    want = fedprox_update([p.cpu().numpy() for p in params], [g.cpu().numpy() for g in glob], 0.05, 0.1)
    kx.prox_update(params, glob, float(0.05 * 0.1))
    for p, w in zip(params, want):
        assert np.array_equal(p.cpu().numpy(), w)


def _dp_module(sc, device):
    m = sc.meta
    return NamedStateModule(m["names"], sc.list("in", len(m["names"])), m["is_param"]).to(device)


@pytest.mark.parametrize("name", [n for n in scenario_names("client") if "_dp_" in n])
def test_local_dp_matches_reference_fixture(gpu_device, name):
    from fedscale_amd import kernels as kx
    from fedscale_amd.cloud.execution.local_dp import _UploadLayout, privatize_update

    sc = ClientScenario(name)
    m = sc.meta
    names, T = m["names"], len(m["names"])
    if m["norm_type"] != 2.0:
        # customized_client.py always clips by the 2-norm; drive the inf fixture through clip_grad_norm_ as
        # the reference generator did (delta = p - last; clip; p = last + delta) — exact: max is exact
        from fedscale_amd.cloud.execution.local_dp import clip_grad_norm_

        pidx = [j for j, f in enumerate(m["is_param"]) if f]
        last = [torch.from_numpy(a).to(gpu_device) for a in sc.list("last", len(pidx))]
        deltas = [torch.from_numpy(sc.arrays[f"in/{j}"]).to(gpu_device) - l for j, l in zip(pidx, last)]
        total = clip_grad_norm_(deltas, m["clip"], m["norm_type"])
        assert np.float32(total.item()) == np.float32(m["total_norm"])
        for j, l, d in zip(pidx, last, deltas):
            assert np.array_equal((l + d).cpu().numpy(), sc.arrays[f"recovered/{j}"])
        return
    model = _dp_module(sc, gpu_device)
    last = [torch.from_numpy(a).to(gpu_device) for a in sc.list("last", sum(m["is_param"]))]
    seed = 1234
    up = privatize_update(model, last, m["clip"], m["noise_factor"], seed=seed)
    assert list(up.keys()) == names
    sigma = np.float32(m["noise_factor"] * m["clip"])
    lay = _UploadLayout(model)
    clipped = m["total_norm"] > m["clip"]
    sd = model.state_dict()
    for j, n in enumerate(names):
        want_rec = sc.arrays[f"recovered/{j}"]
        rec = sd[n].cpu().numpy()
        if want_rec.dtype == np.float32 and m["is_param"][j] and clipped:
            scale = max(float(np.abs(want_rec).max()), 1e-30)
            assert np.max(np.abs(rec.astype(np.float64) - want_rec)) <= 1e-6 * scale, n
        else:
            assert np.array_equal(rec, want_rec), n
        # upload = recovered + own noise, exactly
        z = torch.empty(lay.numel[j], dtype=torch.float32, device=gpu_device)
        kx.dp_normals(z, seed, lay.noise_off[j])
        noise = (z.cpu().numpy() * sigma + np.float32(0)).reshape(lay.shapes[j])
        want_up = np.asarray(rec + noise) if rec.dtype == np.float32 else np.asarray(rec + noise.astype(np.float32))
        assert up[n].dtype == sc.arrays[f"upload/{j}"].dtype, n
        assert up[n].shape == want_up.shape and np.array_equal(up[n], want_up), n


@pytest.mark.parametrize("norm_type", [2.0, float("inf")])
def test_clip_grad_norm_matches_reference_formula(gpu_device, norm_type):
    from fedscale_amd.cloud.execution.local_dp import clip_grad_norm_
    from oracle.cpu_reference import dp_clip_coef

    rng = np.random.default_rng(9)
    ts = _ragged_list(rng, 60, gpu_device)
    if norm_type == float("inf"):  # the reference's abs().max() raises on an empty tensor; so does the device
        with pytest.raises(RuntimeError):
            dp_clip_coef([t.cpu().numpy() for t in ts], 1.0, norm_type)
        with pytest.raises(RuntimeError):
            clip_grad_norm_(ts, 1.0, norm_type)
        ts = [t for t in ts if t.numel()]
    host = [t.cpu().numpy().copy() for t in ts]
    max_norm = 1.0 if norm_type == 2.0 else 0.1
    total_ref, coef_ref, apply_ref = dp_clip_coef(host, max_norm, norm_type)
    assert apply_ref
    total = clip_grad_norm_(ts, max_norm, norm_type)
    assert abs(float(total) - float(total_ref)) <= 1e-6 * float(total_ref)
    for t, h in zip(ts, host):
        want = h * coef_ref
        got = t.cpu().numpy()
        assert np.max(np.abs(got.astype(np.float64) - want), initial=0) <= 2e-6 * max(float(np.abs(want).max(initial=0)), 1e-30)
    # below the threshold nothing moves
    before = [t.clone() for t in ts]
    clip_grad_norm_(ts, 1e9, norm_type)
    assert all(torch.equal(a, b) for a, b in zip(ts, before))


def test_clip_grad_norm_nonfinite_behaviour(gpu_device):
    """NaN total: clip_coef is NaN, `coef < 1` is False, nothing is scaled (clip_norm.py:42-52)."""
    from fedscale_amd.cloud.execution.local_dp import clip_grad_norm_

    t = torch.tensor([1.0, float("nan"), 2.0], device=gpu_device)
    u = torch.tensor([3.0, 4.0], device=gpu_device)
    total = clip_grad_norm_([t, u], 0.5)
    assert torch.isnan(total)
    assert torch.equal(u.cpu(), torch.tensor([3.0, 4.0]))
    with pytest.raises(RuntimeError):
        clip_grad_norm_([t], 0.5, error_if_nonfinite=True)


def test_dp_noise_stream_statistics(gpu_device):
    """The counter-based N(0,1): moments, tail mass and independence of neighbouring draws / seeds."""
    from fedscale_amd import kernels as kx

    n = 1 << 22
    z = kx.dp_normals(torch.empty(n, dtype=torch.float32, device=gpu_device), seed=77).double()
    se = 1.0 / np.sqrt(n)
    assert abs(float(z.mean())) < 6 * se
    assert abs(float(z.std()) - 1.0) < 6 * se
    assert abs(float((z.abs() <= 1.0).double().mean()) - 0.682689) < 6 * 0.47 * se
    assert abs(float((z ** 4).mean()) - 3.0) < 6 * np.sqrt(96) * se
    assert abs(float((z[:-1] * z[1:]).mean())) < 6 * se  # neighbours (the Box-Muller pair) uncorrelated
    z2 = kx.dp_normals(torch.empty(n, dtype=torch.float32, device=gpu_device), seed=78).double()
    assert abs(float((z * z2).mean())) < 6 * se
    off = kx.dp_normals(torch.empty(1000, dtype=torch.float32, device=gpu_device), seed=77, noise_offset=4096)
    assert torch.equal(off.double(), z[4096:5096])  # offsets address the same stream


def test_dp_sigma_zero_is_exact_recover(gpu_device):
    """noise_factor 0: the upload is the recovered state plus +0.0 (int64 entries promoted to float64)."""
    from fedscale_amd.cloud.execution.local_dp import privatize_update

    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.BatchNorm1d(7)).to(gpu_device)
    last = [p.data.clone() for p in net.parameters()]
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.01)
    up = privatize_update(net, last, clip_threshold=100.0, noise_factor=0.0)
    for (n, t), (n2, u) in zip(net.state_dict().items(), up.items()):
        assert n == n2
        h = t.cpu().numpy()
        if h.dtype == np.int64:
            assert u.dtype == np.float64 and np.array_equal(u, h.astype(np.float64))
        else:
            assert u.dtype == np.float32 and np.array_equal(u, h + np.float32(0))


def test_prox_plan_cache_revalidates(gpu_device):
    """A cached pointer table is reused only for the same pointers, sizes, dtypes and contiguity."""
    from fedscale_amd import kernels as kx

    a = torch.ones(4, 6, device=gpu_device)
    g = torch.zeros(4, 6, device=gpu_device)
    kx.prox_update([a], [g], 0.5)
    kx.prox_update([a], [g], 0.5)  # cached
    assert torch.equal(a, torch.full((4, 6), 2.25, device=gpu_device))
    with pytest.raises(ValueError, match="contiguous"):
        kx.prox_update([a.t()], [g], 0.5)
    with pytest.raises(ValueError, match="device tensor"):
        kx.prox_update([a.cpu()], [g.cpu()], 0.5)
    with pytest.raises(TypeError, match="dtype"):
        kx.prox_update([a.double()], [g], 0.5)
    with pytest.raises(ValueError, match="shape"):
        kx.prox_update([a], [torch.zeros(24, device=gpu_device)], 0.5)


def test_client_optimizer_on_a_real_module(gpu_device):
    """ClientOptimizer.update_client_weight after real optimizer steps, against the reference formula."""
    import argparse

    from fedscale_amd.cloud.execution.optimizers import ClientOptimizer
    from oracle.cpu_reference import fedprox_update

    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Flatten(),
                              torch.nn.Linear(4 * 6 * 6, 5)).to(gpu_device)
    glob = [p.data.clone() for p in net.parameters()]
    sgd = torch.optim.SGD(net.parameters(), lr=0.1)
    conf = argparse.Namespace(gradient_policy="fed-prox", learning_rate=0.1, proxy_mu=0.5)
    opt = ClientOptimizer()
    for _ in range(3):
        sgd.zero_grad()
        net(torch.randn(2, 3, 8, 8, device=gpu_device)).square().mean().backward()
        sgd.step()
        before = [p.data.cpu().numpy() for p in net.parameters()]
        opt.update_client_weight(conf, net, glob)
        want = fedprox_update(before, [g.cpu().numpy() for g in glob], 0.1, 0.5)
        for p, w in zip(net.parameters(), want):
            assert np.array_equal(p.data.cpu().numpy(), w)
    conf.gradient_policy = "fed-avg"  # any other policy: no-op
    snap = [p.data.clone() for p in net.parameters()]
    opt.update_client_weight(conf, net, glob)
    assert all(torch.equal(a, b.data) for a, b in zip(snap, net.parameters()))


def _sgd_model(seed, device):
    g = torch.Generator().manual_seed(seed)
    shapes = [(64, 3, 3, 3), (64,), (10, 4097), (10,), (5, 7), (3,)]  # ragged, non-multiple-of-4 tails
    m = torch.nn.Module()
    for i, s in enumerate(shapes):
        m.register_parameter(f"p{i}", torch.nn.Parameter(torch.randn(s, generator=g).to(device)))
    return m, g


@pytest.mark.parametrize("momentum,nesterov,wd,damp", [(0.9, False, 5e-4, 0.0), (0.0, False, 5e-4, 0.0),
                                                       (0.9, True, 1e-3, 0.0), (0.5, False, 0.0, 0.1)])
def test_fused_sgd_prox_step_matches_torch_sgd_then_fedprox(gpu_device, momentum, nesterov, wd, damp):
    """ClientOptimizer.step_and_update == torch.optim.SGD.step() + update_client_weight (torch_client.py:
    236-240, optimizers.py:6-10) over 4 local steps, one parameter without a gradient: parameters and
    momentum buffers within the north-star fp32 tolerance (rtol 1e-5, atol 1e-6) for both variants,
    bit-exact to torch's foreach SGD on the GPU with fma (the default: torch's alpha-adds are contracted), and
    with fma=False bit-exact to the CPU oracle's separately rounded step (oracle.cpu_reference.sgd_prox_step_ref)."""
    import argparse
    import copy

    from fedscale_amd.cloud.execution.optimizers import ClientOptimizer
    from oracle.cpu_reference import fedprox_update, sgd_prox_step_ref

    conf = argparse.Namespace(gradient_policy="fed-prox", learning_rate=0.05, proxy_mu=0.1)
    ref, g = _sgd_model(7, gpu_device)
    glob = [p.detach().clone() + 0.01 for p in ref.parameters()]
    exact = {}
    for fma in (True, False):
        ours = copy.deepcopy(ref)
        r = copy.deepcopy(ref)
        kw = dict(lr=conf.learning_rate, momentum=momentum, weight_decay=wd, nesterov=nesterov, dampening=damp)
        opt_r, opt_o = torch.optim.SGD(r.parameters(), **kw), torch.optim.SGD(ours.parameters(), **kw)
        gg = torch.Generator().manual_seed(11)
        host_p = [p.detach().cpu().numpy().copy() for p in ref.parameters()]  # the CPU oracle's state
        host_m = [None] * len(host_p)
        for step in range(4):
            for i, (pr, po) in enumerate(zip(r.parameters(), ours.parameters())):
                if i == 3:  # no gradient: SGD skips it, FedProx still moves it
                    pr.grad = po.grad = None
                    host_p[i] = fedprox_update([host_p[i]], [glob[i].cpu().numpy()], conf.learning_rate,
                                               conf.proxy_mu)[0]
                    continue
                gr = torch.randn(pr.shape, generator=gg)
                flags = [(1 if nesterov else 0) | (2 if step == 0 else 0)]
                (host_p[i],), (host_m[i],) = sgd_prox_step_ref(
                    [host_p[i]], [gr.numpy()], [host_m[i]], [glob[i].cpu().numpy()], [conf.learning_rate],
                    [momentum], [damp], [wd], flags, np.float32(conf.learning_rate * conf.proxy_mu), False)
                gr = gr.to(gpu_device)
                pr.grad, po.grad = gr.clone(), gr.clone()
            opt_r.step()
            for idx, param in enumerate(r.parameters()):  # optimizers.py:8-10, literally
                param.data += conf.learning_rate * conf.proxy_mu * (param.data - glob[idx])
            ClientOptimizer().step_and_update(opt_o, conf, ours, glob, fma=fma)
        torch.cuda.synchronize()
        ok = True
        for pr, po in zip(r.parameters(), ours.parameters()):
            torch.testing.assert_close(po.detach(), pr.detach(), rtol=1e-5, atol=1e-6)
            ok &= torch.equal(po.detach(), pr.detach())
            if momentum != 0 and pr.grad is not None:
                br, bo = opt_r.state[pr]["momentum_buffer"], opt_o.state[po]["momentum_buffer"]
                torch.testing.assert_close(bo, br, rtol=1e-5, atol=1e-6)
                ok &= torch.equal(bo, br)
        exact[fma] = ok
        if not fma:
            for i, po in enumerate(ours.parameters()):
                assert np.array_equal(po.detach().cpu().numpy().view(np.uint32), host_p[i].view(np.uint32)), i
                if host_m[i] is not None:
                    bo = opt_o.state[po]["momentum_buffer"].cpu().numpy()
                    assert np.array_equal(bo.view(np.uint32), host_m[i].view(np.uint32)), i
    assert exact[True], "fma variant: expected bit-exact to torch SGD + FedProx on the GPU"
    print(f"[sgd-prox] momentum={momentum} nesterov={nesterov} wd={wd} damp={damp}: bit-exact vs torch on GPU "
          f"fma={exact[True]} rounded={exact[False]}")


def test_fused_sgd_prox_step_groups_and_late_gradients(gpu_device):
    """Several param groups with their own lr / weight_decay / momentum / dampening (the detection task
    builds one group per parameter, torch_client.py:100-108), and a parameter whose first gradient comes at
    step 2 (one group then holds first-step and later-step momentum buffers: two launches). Bit-exact to
    torch.optim.SGD.step() + the reference's FedProx lines on the GPU."""
    import argparse
    import copy

    from fedscale_amd.cloud.execution.optimizers import ClientOptimizer

    conf = argparse.Namespace(gradient_policy="fed-prox", learning_rate=0.05, proxy_mu=0.1)
    ref, _ = _sgd_model(9, gpu_device)
    glob = [p.detach().clone() - 0.02 for p in ref.parameters()]
    ours = copy.deepcopy(ref)

    def groups(m):
        ps = list(m.parameters())
        return [dict(params=[ps[0], ps[3]], lr=0.05, momentum=0.9, weight_decay=5e-4, dampening=0.3),
                dict(params=[ps[1]], lr=0.01, momentum=0.0, weight_decay=1e-3),
                dict(params=[ps[2], ps[4]], lr=0.2, momentum=0.7, weight_decay=0.0, dampening=0.05),
                dict(params=[ps[5]], lr=0.03, momentum=0.9, nesterov=True, weight_decay=1e-4)]

    opt_r, opt_o = torch.optim.SGD(groups(ref), lr=0.1), torch.optim.SGD(groups(ours), lr=0.1)
    gg = torch.Generator().manual_seed(3)
    for step in range(5):
        for i, (pr, po) in enumerate(zip(ref.parameters(), ours.parameters())):
            if i == 3 and step < 2:  # no gradient yet: SGD skips it, FedProx still moves it
                pr.grad = po.grad = None
                continue
            gr = torch.randn(pr.shape, generator=gg).to(gpu_device)
            pr.grad, po.grad = gr.clone(), gr.clone()
        opt_r.step()
        for idx, param in enumerate(ref.parameters()):  # optimizers.py:8-10, literally
            param.data += conf.learning_rate * conf.proxy_mu * (param.data - glob[idx])
        ClientOptimizer().step_and_update(opt_o, conf, ours, glob)
        torch.cuda.synchronize()
        for pr, po in zip(ref.parameters(), ours.parameters()):
            assert torch.equal(po.detach(), pr.detach()), f"step {step}: parameter differs"
            br, bo = opt_r.state[pr].get("momentum_buffer"), opt_o.state[po].get("momentum_buffer")
            assert (br is None) == (bo is None)
            if br is not None:
                assert torch.equal(bo, br), f"step {step}: momentum buffer differs"


def test_failed_fused_step_leaves_optimizer_state_unchanged(gpu_device):
    """A launch the library rejects (nesterov with dampening, set on the group after construction) raises
    and leaves no uninitialised momentum buffer in optimizer.state (a later step would read it)."""
    import argparse

    from fedscale_amd._native import FedAggError
    from fedscale_amd.cloud.execution.optimizers import ClientOptimizer

    conf = argparse.Namespace(gradient_policy="fed-prox", learning_rate=0.05, proxy_mu=0.1)
    m, _ = _sgd_model(4, gpu_device)
    glob = [p.detach().clone() for p in m.parameters()]
    opt = torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9, nesterov=True)
    opt.param_groups[0]["dampening"] = 0.5
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    with pytest.raises(FedAggError, match="nesterov"):
        ClientOptimizer().step_and_update(opt, conf, m, glob)
    assert all("momentum_buffer" not in opt.state[p] for p in m.parameters())


def test_fused_step_falls_back_for_tensors_it_does_not_cover(gpu_device):
    """channels_last parameters and params outside model.parameters() take optimizer.step() +
    update_client_weight (the reference's two calls), with the same result as torch."""
    import argparse
    import copy

    from fedscale_amd.cloud.execution.optimizers import ClientOptimizer

    conf = argparse.Namespace(gradient_policy="fed-avg", learning_rate=0.05, proxy_mu=0.1)
    ref = torch.nn.Conv2d(8, 8, 3).to(gpu_device).to(memory_format=torch.channels_last)
    ours = copy.deepcopy(ref)
    assert not ref.weight.is_contiguous()
    opt_r = torch.optim.SGD(ref.parameters(), lr=0.1, momentum=0.9)
    opt_o = torch.optim.SGD(ours.parameters(), lr=0.1, momentum=0.9)
    for _ in range(2):
        for pr, po in zip(ref.parameters(), ours.parameters()):
            g = torch.randn_like(pr)
            pr.grad, po.grad = g.clone(), g.clone()
        opt_r.step()
        ClientOptimizer().step_and_update(opt_o, conf, ours, None)
    for pr, po in zip(ref.parameters(), ours.parameters()):
        assert torch.equal(pr, po)


def test_persistent_client_optimizer_reuses_its_step_plan(gpu_device, monkeypatch):
    """The executor keeps one ClientOptimizer (torch_client.py:26): from the second local step on, the fused
    step runs from its cached tables (fa_sgd_prox_step_groups on the plan's pointers) and stays bit-exact to
    torch's SGD + FedProx through an lr schedule, a momentum change, fresh gradient tensors every step
    (zero_grad(set_to_none=True)), a new round's global model and optimizer.load_state_dict."""
    import argparse
    import copy

    from fedscale_amd import kernels as kx
    from fedscale_amd.cloud.execution.optimizers import ClientOptimizer

    calls = {"general": 0, "plan": 0}
    gen, raw = kx.sgd_prox_step_groups, kx.sgd_prox_step_groups_raw

    def count(kind, f):
        def w(*a, **k):
            calls[kind] += 1
            return f(*a, **k)
        return w

    monkeypatch.setattr(kx, "sgd_prox_step_groups", count("general", gen))
    monkeypatch.setattr(kx, "sgd_prox_step_groups_raw", count("plan", raw))
    conf = argparse.Namespace(gradient_policy="fed-prox", learning_rate=0.05, proxy_mu=0.1)
    ref, _ = _sgd_model(21, gpu_device)
    ours = copy.deepcopy(ref)
    kw = dict(lr=0.05, momentum=0.9, weight_decay=5e-4)
    opt_r, opt_o = torch.optim.SGD(ref.parameters(), **kw), torch.optim.SGD(ours.parameters(), **kw)
    sch_r = torch.optim.lr_scheduler.StepLR(opt_r, step_size=2, gamma=0.5)
    sch_o = torch.optim.lr_scheduler.StepLR(opt_o, step_size=2, gamma=0.5)
    co = ClientOptimizer()
    gg = torch.Generator().manual_seed(5)
    glob = None
    trace = []
    for step in range(10):
        if step % 4 == 0:  # a new round: a new global model list (torch_client.py: one per train())
            glob = [p.detach().clone() + 0.01 * (step + 1) for p in ref.parameters()]
        if step == 5:  # momentum changes mid-run (still non-zero): the plan reads it per step
            for o in (opt_r, opt_o):
                o.param_groups[0]["momentum"] = 0.8
        if step == 7:  # state replaced wholesale
            opt_o.load_state_dict(copy.deepcopy(opt_r.state_dict()))
        for pr, po in zip(ref.parameters(), ours.parameters()):
            gr = torch.randn(pr.shape, generator=gg).to(gpu_device)
            pr.grad, po.grad = gr.clone(), gr.clone()  # new gradient tensors every step
        opt_r.step()
        for idx, param in enumerate(ref.parameters()):  # optimizers.py:8-10, literally
            param.data += conf.learning_rate * conf.proxy_mu * (param.data - glob[idx])
        before = dict(calls)
        co.step_and_update(opt_o, conf, ours, glob)
        trace.append("plan" if calls["plan"] > before["plan"] else "general")
        sch_r.step()
        sch_o.step()
        torch.cuda.synchronize()
        for pr, po in zip(ref.parameters(), ours.parameters()):
            assert torch.equal(po.detach(), pr.detach()), f"step {step}: parameter differs"
            assert torch.equal(opt_o.state[po]["momentum_buffer"], opt_r.state[pr]["momentum_buffer"]), step
    # general launches: step 0 (first step), 4 and 8 (new global models), 7 (state replaced); the rest from
    # the plan
    assert trace == ["general", "plan", "plan", "plan", "general", "plan", "plan", "general", "general", "plan"], trace
