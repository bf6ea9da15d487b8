"""Auxo gradient-signature fixtures from the REAL reference (build container only; needs /root/reference).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_auxo_sig.py

For every fixture the reference's own ``AuxoClientMetadata.register_gradient``
(examples/auxo/client_metadata.py:10-17) is called per upload with ``W`` = the upload dict and ``W_old`` = the
cohort model's tensors, exactly as examples/auxo/aggregator.py:293-302 reaches it through ``register_feedback``;
then the three lines of ``cohort_clustering`` that make the clustering features are applied to its outputs
(client_manager.py:208-210: ``np.mean(gradient_list, axis=0)``, ``gradient_list - avg_grad``,
``sklearn.preprocessing.normalize``).  Outputs are data only — the model, the K uploads and the recorded
results — one ``auxo_sig_<name>.npz`` each (tests/cohort_sig_fixtures.py loads them); no reference text is kept.

Fixtures
    mixed_k9        fp32 tensors of odd sizes and two int64 0-d buffers, one inside the tail; unrounded fp32 noise
    femnist_cnn_k10 config 1's small-CNN layout (P = 24,492); uploads stored as int8 steps of 2^-10 (file size)
    tiny_k5         Linear(1, 1): N = 2 < 10, so val_len = 0 and ``gradient[-0:]`` is the whole vector
    values_k6       crafted differences: float16 subnormals, exact ties, overflow to +-inf, int64 steps <= 2048
"""
from __future__ import annotations

import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gen_golden as G  # noqa: E402  (the reference import's placeholders, FemnistCNN)
from tests.cohort_sig_fixtures import SigFixture  # noqa: E402


def _import_auxo():
    sys.argv = [sys.argv[0]]
    sys.path.insert(0, G.REF)
    sys.path.insert(0, os.path.join(G.REF, "examples", "auxo"))
    G._install_placeholders()
    from client_metadata import AuxoClientMetadata  # examples/auxo/client_metadata.py

    return AuxoClientMetadata


def _reference_features(Meta, fx: SigFixture) -> dict:
    from sklearn import preprocessing

    w_old = [torch.from_numpy(np.array(m)) for m in fx.model]  # model_wrapper.get_weights(): CPU tensors
    gradient_list = []
    for k in range(fx.K):
        md = Meta(0, k + 1, {"computation": 1.0, "communication": 1.0})
        gradient_list.append(md.register_gradient(fx.upload(k), w_old))
    out = {"sig": np.stack(gradient_list)}
    assert out["sig"].dtype == np.float16
    with np.errstate(invalid="ignore", over="ignore"):
        avg_grad = np.mean(gradient_list, axis=0)           # client_manager.py:208
        centered_grad = gradient_list - avg_grad            # :209
    out["mean"], out["centered"] = avg_grad, centered_grad
    assert avg_grad.dtype == np.float16 and centered_grad.dtype == np.float16
    if np.isfinite(centered_grad).all():
        out["normalized"] = preprocessing.normalize(centered_grad)  # :210
        assert out["normalized"].dtype == np.float16
    return out


def _write(Meta, name, names, model, uploads=None, udelta=None, scale=None):
    arrays = {"names": np.asarray(names)}
    for i, m in enumerate(model):
        arrays[f"model/{i}"] = G._compact(m)  # float16 when that round-trips exactly
    if udelta is not None:
        arrays["udelta_scale"] = np.float32(scale)
        for i, d in enumerate(udelta):
            arrays[f"udelta/{i}"] = d
    else:
        for i, u in enumerate(uploads):
            arrays[f"uploads/{i}"] = u
    fx = SigFixture(name, arrays)  # the uploads exactly as the tests will see them
    arrays.update(_reference_features(Meta, fx))
    path = os.path.join(G.OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"  {name}: K={fx.K} D={arrays['sig'].shape[1]} {os.path.getsize(path) / 1024:.1f} KiB"
          f"{'' if 'normalized' in arrays else ' (non-finite centred matrix: no normalize)'}")


def _noisy(rng, model, K, scale):
    ups = []
    for m in model:
        if m.dtype == np.int64:
            ups.append(m[None] + rng.integers(-2048, 2049, size=(K,) + m.shape))
        else:
            ups.append((m[None] + rng.normal(0.0, scale, size=(K,) + m.shape)).astype(np.float32))
    return ups


def gen_mixed(Meta):
    rng = np.random.default_rng(41)
    spec = [("a.weight", (7, 5), "f"), ("bn.count", (), "i"), ("b.weight", (3, 11), "f"), ("c.bias", (129,), "f"),
            ("e.weight", (13, 17), "f"), ("bn2.count", (), "i"), ("f.bias", (19,), "f")]
    model = [np.asarray(rng.integers(0, 5000), dtype=np.int64) if k == "i" else
             rng.normal(0.0, 0.05, size=s).astype(np.float32) for _, s, k in spec]
    _write(Meta, "auxo_sig_mixed_k9", [n for n, _, _ in spec], model, uploads=_noisy(rng, model, 9, 0.01))


def gen_femnist(Meta):
    torch.manual_seed(7)
    rng = np.random.default_rng(7)
    sd = G.FemnistCNN().state_dict()
    model = [rng.normal(0.0, 0.05, size=tuple(v.shape)).astype(np.float16).astype(np.float32) for v in sd.values()]
    # fc2 (the last 3,162 elements, which hold the 2,449 of the signature): steps of -2 .. 2; the layers before it:
    # a sparse +-1 (they only have to differ from the model, and compress well)
    udelta = [(rng.integers(-2, 3, size=(10,) + m.shape) if i >= len(model) - 2 else
               rng.choice([-1, 0, 0, 0, 0, 0, 0, 1], size=(10,) + m.shape)).astype(np.int8)
              for i, m in enumerate(model)]
    _write(Meta, "auxo_sig_femnist_cnn_k10", list(sd.keys()), model, udelta=udelta, scale=2.0 ** -10)


def gen_tiny(Meta):
    rng = np.random.default_rng(3)
    sd = torch.nn.Linear(1, 1).state_dict()
    model = [rng.normal(0.0, 0.5, size=tuple(v.shape)).astype(np.float32) for v in sd.values()]
    _write(Meta, "auxo_sig_tiny_k5", list(sd.keys()), model, uploads=_noisy(rng, model, 5, 0.1))


def gen_values(Meta):
    """N = 300 + 1 + 30 = 331, D = 33: the tail is v[298:300], the int64 counter and all of w.  The model is 0
    at the crafted positions, so W_old - W is minus the upload there, exactly."""
    rng = np.random.default_rng(11)
    K = 6
    model = [rng.normal(0.0, 0.05, size=(300,)).astype(np.float32), np.asarray(100000, dtype=np.int64),
             np.zeros(30, dtype=np.float32)]
    ups = _noisy(rng, model, K, 0.01)
    ups[1] = model[1] - np.asarray([2048, -2048, 2047, -1025, 0, 1], dtype=np.int64)  # |difference| <= 2048
    w = ups[2]
    sub = 2.0 ** -24  # the smallest float16 subnormal
    crafted = np.asarray([
        [sub, 3 * sub, 0.5 * sub, 1.5 * sub, 2.5 * sub, 1023 * sub],             # subnormals, ties at the bottom
        [-sub, -0.5 * sub, 0.49 * sub, 2.0 ** -14, 2.0 ** -14 - sub, 2.0 ** -15],
        [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2048 + 1, 2048 + 3, 0.1],   # exact ties: to even
        [1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -11 - 2.0 ** -24, 1e-3, -1e-3, 3.1415927, -2.7182817],
        [65504.0, 65519.996, 65520.0, 1e5, -65520.0, -7e4],                     # the float16 range and beyond
        [-65519.996, 3e38, -3e38, 65536.0, 4e4, -4e4],
    ], dtype=np.float64).astype(np.float32)
    for c in range(crafted.shape[0]):   # column c of w holds row c of the table, one value per client
        w[:, c] = -crafted[c]
    w[:, 6] = np.float32(-7e4)           # a column that overflows for every client: inf - inf in the centring
    _write(Meta, "auxo_sig_values_k6", ["v", "count", "w"], model, uploads=ups)


def main():
    Meta = _import_auxo()
    print("auxo signature fixtures:")
    gen_mixed(Meta)
    gen_femnist(Meta)
    gen_tiny(Meta)
    gen_values(Meta)


if __name__ == "__main__":
    main()
