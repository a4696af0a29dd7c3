"""One context per device however the device is named (shapemol_amd/_native.py): 'cuda', 'cuda:0' while device 0 is current and a
tensor's .device reach the same library context in the encoder, the decoder, the shape-data builder and the surface builder, and
what the context computes does not depend on the name."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import shape_data_oracle as SD  # noqa: E402
import shape_decoder_f64 as D  # noqa: E402
import shape_encoder_f64 as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_encoder_has_one_context_for_cuda_and_cuda0():
    import shapemol_amd
    assert torch.cuda.current_device() == 0
    enc = shapemol_amd.VN_DGCNN_Encoder(128, 32, 4, S.K)
    enc.load_state_dict(S.state_dict(4, 32), strict=False)
    enc = enc.to(DEV)
    x = S.clouds(1, 32, 3).to(DEV)                                  # B = 1, N = 32: the smallest the library accepts
    first = enc(x)
    handle = enc._ctx.value
    assert handle
    n_max = enc.max_points("cuda")
    assert enc._ctx.value == handle
    assert enc.max_points(DEV) == n_max and enc._ctx.value == handle
    assert enc.max_points(x.device) == n_max and enc._ctx.value == handle
    second = enc(x)
    assert enc._ctx.value == handle
    assert torch.equal(first, second)


def test_decoder_has_one_context_for_cuda_and_cuda0():
    from shapemol_amd.shape_autoencoder import DecoderInner
    assert torch.cuda.current_device() == 0
    dec = DecoderInner(3, 32, 128, 4, "signeddist")
    dec.load_state_dict(D.state_dict(4, 32), strict=True)
    dec = dec.to(DEV)
    tile = dec.tile(DEV)
    handle = dec._ctx.value
    assert handle
    p, _, z = D.inputs(1, tile, 32, 5)                                # B = 1, one tile of points
    first = dec(p.view(1, tile, 3).to(DEV), z.to(DEV))
    assert dec._ctx.value == handle
    assert dec.tile("cuda") == tile and dec._ctx.value == handle
    assert dec.tile(DEV) == tile and dec._ctx.value == handle
    second = dec(p.view(1, tile, 3).to(DEV), z.to(DEV))
    assert dec._ctx.value == handle
    assert torch.equal(first, second)


def _one_cached_context(contexts):
    a = contexts.of("cuda")
    assert contexts.of(DEV) is a and contexts.of(torch.device(DEV)) is a and contexts.of(torch.device("cuda")) is a
    assert a.value and list(contexts._by_index) == [0]
    return a.value


def test_shape_data_has_one_context_per_device():
    from shapemol_amd import shape_data
    mesh = SD.tetrahedron()
    build = lambda dev: shape_data.build_batch([mesh], 32, 2, "signed_distance", device=dev, seed=11)  # noqa: E731  (P = 32, T = 2)
    first = build(DEV)
    handle = _one_cached_context(shape_data._contexts)
    second = build("cuda")
    assert _one_cached_context(shape_data._contexts) == handle
    assert sorted(first) == sorted(second)
    for k, v in first.items():
        same = torch.equal(v, second[k]) if isinstance(v, torch.Tensor) else np.array_equal(v, second[k])
        assert same, k


def test_mol_surface_has_one_context_per_device():
    from shapemol_amd import mol_surface
    pos, radii = np.array([[0.0, 0.0, 0.0], [1.2, 0.3, -0.2]]), np.array([1.7, 1.52])          # one 2-atom molecule
    first = mol_surface.get_mesh(pos, radii=radii, device=DEV)
    handle = _one_cached_context(mol_surface._contexts)
    second = mol_surface.get_mesh(pos, radii=radii, device="cuda")
    assert _one_cached_context(mol_surface._contexts) == handle
    assert len(first[0]) > 0 and len(first[1]) > 0
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
