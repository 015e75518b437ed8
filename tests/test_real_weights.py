"""Real-weight vectors (tests/golden/real_weights_b16.npz, written by oracle/gen_golden_real.py from the reference's own
functions on the reference's own tensors): the CPU restatement must reproduce them bit for bit, and this repo's
load_weights() must find the 116 blobs of a tree named like the reference's (tests/golden/real_weights_manifest.json).

End-to-end real-weight parity stays UNPINNED: Data/input-100.bin and the 36 in_proj / fc1 / fc2 weight blobs are absent
upstream, so answer_result.txt cannot be reproduced by anyone from this tree.
"""
import glob
import hashlib
import json
import os

import numpy as np
import pytest

from vit_amd import binding as B
from vit_amd import synth

GOLD = os.path.join(os.path.dirname(__file__), "golden", "real_weights_b16.npz")
MANIFEST = os.path.join(os.path.dirname(__file__), "golden", "real_weights_manifest.json")   # oracle/gen_golden_real.py
T, D = 197, 768


def load_gold():
    """GOLD as a dict, its large tensors put back together from the row blocks in real_weights_b16.partNN.npz
    (oracle/gen_golden_real.py: save_split)."""
    with np.load(GOLD) as z:
        g = {k: z[k] for k in z.files}
    blocks = {}
    for path in sorted(glob.glob(GOLD[:-len(".npz")] + ".part*.npz")):
        with np.load(path) as z:
            for key in z.files:
                name, j = key.rsplit(".", 1)
                blocks.setdefault(name, {})[int(j)] = z[key]
    for name, b in blocks.items():
        g[name] = np.concatenate([b[j] for j in range(len(b))])
    return g


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


def outlier_cols(x, cols, scale):
    x = x.copy()
    x[:, cols] *= np.float32(scale)
    return x


def activation_inputs(seed, layer):
    """Same streams as oracle/gen_golden_real.py."""
    a = synth.uniform(seed, 100 + layer, T * D, -1.0, 1.0).reshape(T, D)
    x = synth.uniform(seed, 200 + layer, T * D, -2.0, 2.0).reshape(T, D)
    return outlier_cols(a, [7, 300, 301, 640], 12.0), outlier_cols(x, [5, 381, 759], 30.0)


def head_input(seed):
    return outlier_cols(synth.uniform(seed, 300, T * D, -2.0, 2.0).reshape(T, D), [5, 381, 759], 30.0)


def sha256_f32(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def test_loader_reproduces_the_116_real_blobs_and_the_fixture_holds_them(tmp_path):
    """The reference's Network/ directory, laid out from MANIFEST (its 116 file names and sizes) with seeded stand-in
    contents: the loader finds exactly those blobs, each of the size the index map gives and rounded as Network.c:184-187
    does; and the real tensors the fixture stores are those blobs after that rounding (their digests in MANIFEST)."""
    cfg = synth.VIT_B16
    with open(MANIFEST) as f:
        m = json.load(f)
    raws = {}
    for e in m["files"]:
        i = e["index"]
        assert e["name"].startswith(f"Weight_{i}_") and e["name"].endswith(".bin")
        raws[i] = synth.uniform(4321, i, e["floats"], -0.6, 0.6)
        raws[i].astype("<f4").tofile(tmp_path / e["name"])
    W = B.load_weight_dir(str(tmp_path), cfg.n_weights)
    present = [i for i, w in enumerate(W) if w is not None]
    assert present == sorted(raws) and len(present) == 116
    shapes = cfg.weight_shapes()
    L = B.lib()
    cc = B.CConfig.of(cfg)
    import ctypes as C
    for i in present:
        assert raws[i].size == L.vit_config_weight_size(C.byref(cc), i) == int(np.prod(shapes[i]))
        assert same_bits(W[i], synth.round6(raws[i]))             # Network.c:184-187: roundf(w * 1e6f) / 1e6f
    assert all((i - 4) % 12 in (2, 8, 10) for i in set(range(152)) - set(present))   # in_proj / fc1 / fc2 weights
    digest = {e["index"]: e["round6_sha256"] for e in m["files"]}
    g = load_gold()
    assert list(g["present"]) == present
    for i in range(6):
        assert sha256_f32(g[f"w{i}"]) == digest[i]
    for l in g["outproj_layers"]:
        b = 4 + 12 * int(l)
        assert sha256_f32(g[f"outproj_w_{l}"]) == digest[b + 4] and sha256_f32(g[f"ln2_w_{l}"]) == digest[b + 6]
    assert int(g["head_classes"]) == m["head_w_rows"] and sha256_f32(g["head_w"]) == m["head_w_rows_round6_sha256"]
    assert sha256_f32(g["ln_w"]) == digest[148]


def test_restatement_matches_real_weight_vectors(oracle):
    from conftest import oracle_config
    g = load_gold()
    seed, rows = int(g["seed"]), list(g["rows"])
    cfg = synth.VIT_B16
    image = synth.make_images(cfg, 1, seed)[0]
    w = [g[f"w{i}"] for i in range(6)]
    x = oracle.embed(oracle_config(cfg), image, w)
    assert same_bits(x[rows], g["embed_rows"]) and x.astype(np.float64).sum() == float(g["embed_sum"])
    y = oracle.layer_norm(x, w[4], w[5])
    assert same_bits(y[rows], g["ln1_rows"]) and y.astype(np.float64).sum() == float(g["ln1_sum"])
    for l in g["outproj_layers"]:
        a, xres = activation_inputs(seed, int(l))
        r = xres + oracle.linear(a, g[f"outproj_w_{l}"], g[f"outproj_b_{l}"])
        assert same_bits(r[rows], g[f"resid_rows_{l}"]) and r.astype(np.float64).sum() == float(g[f"resid_sum_{l}"])
        assert same_bits(oracle.layer_norm(r, g[f"ln2_w_{l}"], g[f"ln2_b_{l}"])[rows], g[f"ln2_rows_{l}"])
    z = oracle.layer_norm(head_input(seed), g["ln_w"], g["ln_b"])[:8]
    assert same_bits(z, g["final_ln"])
    assert same_bits(oracle.linear(np.ascontiguousarray(z), g["head_w"], g["head_b"]), g["head_logits"])
