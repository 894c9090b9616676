"""Writes tests/golden/classifier_*.npz: the unmodified reference EGNN property classifier (src/__init__.py EGNN, imported under
ref_harness.install_stubs()) on synthetic weights and seeded inputs, four configurations.

Each fixture holds data only: the ragged inputs (num_nodes, x, one_hot), the reference's prediction in fp32 and fp64, h after the embedding
and after every layer in fp64 (forward hooks), the fp32-vs-fp64 distance of the prediction (`gap`) and of every layer (`gap_layers`), and the
state-dict key / shape list as JSON.  Weights are synth.make_weights(shapes, seed=11) keyed by the state-dict names, so none are stored.
The reference is fed its own dense layout (padded rows, node mask, edge mask, full adjacency); real rows are picked out for the fixture.

    python tests/golden/make_classifier_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh                      # noqa: E402
import synth                                  # noqa: E402
import classifier_ref as cr                   # noqa: E402

SIZES64 = [3 + (7 * k) % 27 for k in range(64)]          # 64 molecules, sizes 3 .. 29
CONFIGS = {
    # name: hidden_nf, n_layers, attention, node_attr, sizes
    "h128_l7_att": (128, 7, 1, 0, SIZES64),
    "h128_l7_attr": (128, 7, 0, 1, SIZES64),
    "h64_l2_att_attr": (64, 2, 1, 1, SIZES64),
    "h256_l1": (256, 1, 0, 0, [29, 3, 17, 8, 23, 12, 5, 19]),
}
F, WEIGHT_SEED, INPUT_SEED = 5, 11, 5


def run_reference(src, W, H, L, att, attr, x, h0, sizes, dtype):
    model = src.EGNN(in_node_nf=F, in_edge_nf=0, hidden_nf=H, device="cpu", n_layers=L, coords_weight=1.0, attention=att, node_attr=attr)
    model.load_state_dict(W)
    model = model.to(dtype).eval()
    xp, hp, nm, em, n = cr.to_padded(x, h0, sizes)
    edges = src.get_classifier_adj_matrix(n, len(sizes), "cpu", edges_dic={})
    hs = []
    hooks = [model.embedding.register_forward_hook(lambda m, i, o: hs.append(o.detach().clone()))]
    for k in range(L):
        hooks.append(model._modules[f"gcl_{k}"].register_forward_hook(lambda m, i, o: hs.append(o[0].detach().clone())))
    with torch.no_grad():
        pred = model(h0=hp.to(dtype), x=xp.to(dtype), edges=edges, edge_attr=None, node_mask=nm.to(dtype), edge_mask=em.to(dtype), n_nodes=n)
    for h in hooks:
        h.remove()
    real = nm.reshape(-1) != 0
    return pred, [h[real] for h in hs], list(model.state_dict().items())


def main():
    assert rh.reference_available(), "reference checkout not found"
    rh.install_stubs()
    import importlib
    src = importlib.import_module("src")
    for name, (H, L, att, attr, sizes) in CONFIGS.items():
        shapes = cr.state_dict_shapes(F, H, L, bool(att), bool(attr))
        W = synth.make_weights(shapes, seed=WEIGHT_SEED)
        x, h0 = cr.make_batch(sizes, F, seed=INPUT_SEED)
        p32, h32, sd = run_reference(src, W, H, L, att, attr, x, h0, sizes, torch.float32)
        p64, h64, _ = run_reference(src, W, H, L, att, attr, x, h0, sizes, torch.float64)
        assert [(k, tuple(v.shape)) for k, v in sd] == [(k, tuple(s)) for k, s in shapes.items()], "state-dict layout differs from the reference"
        gap = float((p32.double() - p64).abs().max())
        gap_layers = [float((a.double() - b).abs().max()) for a, b in zip(h32, h64)]
        out = dict(num_nodes=np.array(sizes, dtype=np.int64), x=x.numpy(), one_hot=h0.numpy(), pred32=p32.numpy(), pred64=p64.numpy(),
                   gap=np.float64(gap), gap_layers=np.array(gap_layers), config=np.array([F, H, L, att, attr], dtype=np.int64),
                   state_dict=np.array(json.dumps([[k, list(v.shape)] for k, v in sd])))
        # h of every layer in fp64 for every atom is too large for the 128-wide cases: keep the first 6 molecules' rows (sizes 3 .. 29 occur)
        rows = int(sum(sizes[:6])) if len(sizes) > 8 else int(sum(sizes))
        out["layer_rows"] = np.int64(rows)
        out["h_layers"] = np.stack([h[:rows].numpy() for h in h64])
        gap_rows = [float((a[:rows].double() - b[:rows]).abs().max()) for a, b in zip(h32, h64)]
        out["gap_layers"] = np.array(gap_rows)
        path = os.path.join(HERE, f"classifier_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{name}: max|p| = {float(p64.abs().max()):.3g}  gap = {gap:.2e}  layer gaps {min(gap_rows):.1e} .. {max(gap_rows):.1e}  "
              f"{os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
