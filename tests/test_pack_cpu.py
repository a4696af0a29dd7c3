"""The device weight image built by csrc/sm_pack.h, without a GPU.

tests/pack_probe.cpp includes sm_pack.h, builds the image of a model's packed weights and reports its size, hid_max and every
DevModel / DevLayer offset; the image bytes are hashed here.  The expected values (tests/golden/pack_image.json) were recorded
with this same probe from the packer as it stood before it was restructured (the code moved into sm_pack.h verbatim).
UPDATE_PACK_GOLDEN=1 rewrites the fixture."""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from util import GOLDEN, ROOT, model_cfg, synth

FIXTURE = os.path.join(GOLDEN, "pack_image.json")
CASES = {
    "full": dict(),                                             # the sampling model: H = 128, k as configured
    "reduced_h32": dict(hidden_dim=32, n_heads=4, num_layers=2),     # the reduced model of the GPU tests
    "k32": dict(knn=32, num_layers=2),
}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("pack_probe") / "pack_probe")
    r = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O2", "-o", exe,
                        os.path.join(ROOT, "tests", "pack_probe.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def probe_image(exe, overrides, tmp_path, num_classes=15):
    """(the probe's report, the image as float32, the state dict, the packed weights) of a model with `num_classes` atom types."""
    from shapemol_amd import _lib, pack_state_dict
    from shapemol_amd.spec import ModelDims
    cfg = model_cfg(**overrides)
    d = ModelDims(cfg, num_classes)
    sdn = synth.synthetic_state_dict(cfg, seed=7, num_classes=num_classes)
    packed = pack_state_dict(sdn, d.L)
    conf = _lib.Config(d.H, d.heads, d.L, d.k, d.G, d.S, d.S_latent, d.temb, d.C, d.T)
    src, dst = str(tmp_path / "weights.bin"), str(tmp_path / "image.bin")
    with open(src, "wb") as f:
        f.write(bytes(conf))
        f.write(np.ascontiguousarray(packed, np.float32).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = dict(line.split() for line in r.stdout.splitlines())
    image = open(dst, "rb").read()
    assert len(image) == 4 * int(out["size"])
    return out, image, sdn, packed


def run_probe(exe, overrides, tmp_path, num_classes=15):
    out, image, _, _ = probe_image(exe, overrides, tmp_path, num_classes)
    out["sha256"] = hashlib.sha256(image).hexdigest()
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_image_is_what_the_packer_always_built(probe, case, tmp_path):
    got = run_probe(probe, CASES[case], tmp_path)
    if os.environ.get("UPDATE_PACK_GOLDEN") == "1":
        all_ = json.load(open(FIXTURE)) if os.path.exists(FIXTURE) else {}
        all_[case] = got
        json.dump(all_, open(FIXTURE, "w"), indent=0, sort_keys=True)
    want = json.load(open(FIXTURE))[case]
    assert sorted(got) == sorted(want)
    assert len(got) > 100                    # every offset is reported
    diff = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not diff, diff


@pytest.mark.parametrize("num_classes,nt2", [(10, 1), (16, 1), (17, 2), (23, 2), (32, 2)])
def test_atom_type_head_tiles_and_padding(probe, num_classes, nt2, tmp_path):
    """The atom-type head (v_inference) of a model with another vocabulary: its second Linear is padded to whole 16-row output
    tiles (nt2 of them), the padding rows of weight and bias are zero and the real rows are the state dict's, and the packed
    weight count is what state_dict_spec says (the probe reads exactly shapemol_weight_count floats)."""
    from shapemol_amd.packing import pack_order
    from shapemol_amd.spec import ModelDims, state_dict_spec
    out, image, sdn, packed = probe_image(probe, {}, tmp_path, num_classes)
    cfg = model_cfg()
    d = ModelDims(cfg, num_classes)
    spec = state_dict_spec(d)
    assert packed.size == sum(int(np.prod(spec[k][0])) for k in pack_order(d.L))
    assert spec["v_inference.2.weight"][0] == (num_classes, d.H) and spec["ligand_atom_emb.weight"][0] == (d.H, num_classes + d.temb)
    assert int(out["dm.vhead.nt2"]) == nt2
    im = np.frombuffer(image, np.float32)
    rows, K = 16 * nt2, d.H
    b2 = im[int(out["dm.vhead.b2"]):int(out["dm.vhead.b2"]) + rows]
    assert np.array_equal(b2[:num_classes], sdn["v_inference.2.bias"]) and not b2[num_classes:].any()
    # the A-fragment image of pack_image: element ((t2 * K / 16 + t) * 64 + lane) * 4 + r is W[16 t2 + lane % 16][16 t + 4 (lane / 16) + r]
    frag = im[int(out["dm.vhead.w2img"]):int(out["dm.vhead.w2img"]) + rows * K].reshape(nt2, K // 16, 64, 4)
    t2, t, lane, r = np.meshgrid(np.arange(nt2), np.arange(K // 16), np.arange(64), np.arange(4), indexing="ij")
    w = np.zeros((rows, K), np.float32)
    w[16 * t2 + lane % 16, 16 * t + 4 * (lane // 16) + r] = frag
    assert np.array_equal(w[:num_classes], sdn["v_inference.2.weight"]) and not w[num_classes:].any()
    # the embedding [H][C + D] and its transpose [C + D][H]
    e = num_classes + d.temb
    emb = im[int(out["dm.embw"]):int(out["dm.embw"]) + d.H * e].reshape(d.H, e)
    embT = im[int(out["dm.embwT"]):int(out["dm.embwT"]) + d.H * e].reshape(e, d.H)
    assert np.array_equal(emb, sdn["ligand_atom_emb.weight"]) and np.array_equal(embT, emb.T)


@pytest.mark.parametrize("case", ["h32_k9", "h128_sl36", "h32_max_k32"])
def test_shape_time_and_vocabulary_dimensions_in_the_image(probe, case, tmp_path):
    """Configurations away from S = 32, SL = 32, D = 8, C = 15 (tests/config_space.py), checked structurally against the state
    dict -- not hashed: a hash recorded from the packer proves nothing about a shape it has never been compared at.  Per layer the
    split-off shape columns of each edge MLP's first Linear ([H][SL] = columns G + 2H onwards of net.0.weight) and the two
    VN-linear weights ([heads][1 + heads + S]); the invariant shape MLP ([S][S], [SL][S]), the time MLP ([2D][D], [D][2D]) and the
    embedding [H][C + D] with its transpose."""
    import config_space as CS
    from shapemol_amd.spec import ModelDims
    C = CS.classes(case)
    out, image, sdn, _ = probe_image(probe, CS.overrides(case), tmp_path, C)
    d = ModelDims(CS.config(case), C)
    im = np.frombuffer(image, np.float32)

    def at(name, *shape):
        off = int(out[name])
        return im[off:off + int(np.prod(shape))].reshape(shape)

    assert len(sdn["time_emb.1.weight"]) == 2 * d.temb and sdn["ligand_atom_emb.weight"].shape == (d.H, C + d.temb)
    for l in range(d.L):
        base = f"refine_net.base_block.{l}."
        for dev, key in (("sk_x2h", "x2h_layers.0.hk_func"), ("sv_x2h", "x2h_layers.0.hv_func"), ("sk_h2x", "h2x_layers.0.xk_func"),
                         ("sv_h2x", "h2x_layers.0.xv_func")):
            w = sdn[base + key + ".net.0.weight"]
            assert w.shape == (d.H, d.G + 2 * d.H + d.S_latent)
            assert np.array_equal(at(f"dm.layer{l}.{dev}", d.H, d.S_latent), w[:, d.G + 2 * d.H:]), (l, dev)
        for dev, key in (("vn_f", "map_to_feat"), ("vn_d", "map_to_dir")):
            w = sdn[base + f"h2x_layers.0.shape_linear.{key}.weight"]
            assert w.shape == (d.heads, 1 + d.heads + d.S)
            assert np.array_equal(at(f"dm.layer{l}.{dev}", d.heads, 1 + d.heads + d.S), w), (l, dev)
            assert np.array_equal(at(f"dm.layer{l}.w{dev[-1]}_x", d.heads), w[:, 0]), (l, dev)
    inv = "refine_net.invariant_shape_layer.hidden_layer.net."
    assert np.array_equal(at("dm.inv.w1", d.S, d.S), sdn[inv + "0.weight"]) and np.array_equal(at("dm.inv.w2", d.S_latent, d.S), sdn[inv + "3.weight"])
    assert np.array_equal(at("dm.inv.b2", d.S_latent), sdn[inv + "3.bias"])
    assert np.array_equal(at("dm.te1w", 2 * d.temb, d.temb), sdn["time_emb.1.weight"]) and np.array_equal(at("dm.te2w", d.temb, 2 * d.temb), sdn["time_emb.3.weight"])
    e = C + d.temb
    emb = at("dm.embw", d.H, e)
    assert np.array_equal(emb, sdn["ligand_atom_emb.weight"]) and np.array_equal(at("dm.embwT", e, d.H), emb.T)
    assert int(out["dm.vhead.nt2"]) == (C + 15) // 16
