"""CPU: MeshFeaturizer against the reference's recorded float32 run (tests/golden/fx_featurizer.npz, tools/make_golden_featurizer.py):
parameter names, the neck (positional encoding, heat kernel signatures, multi-view features) and both outputs on the torch route."""
import numpy as np
import pytest
import torch

import lift_checks as lc
from densematcher_amd import diffusion_net
from densematcher_amd.model import MeshFeaturizer


def test_state_dict_keys_are_the_reference_names():
    model, names = lc.featurizer()
    assert list(model.state_dict().keys()) == names
    assert any(n.startswith("extractor_3d.block_1.") for n in names) and "reconstructor.weight" in names
    fx = lc.golden("fx_featurizer.npz")
    assert model.diffusion_in_channels == fx["fts"].shape[1] + 16 + 51 and model.pos_enc_size == 51


def test_reconstructor_variants_build():
    assert isinstance(MeshFeaturizer(num_blocks=1, width=8, num_features=4, reconstructor_layers=3).reconstructor, torch.nn.Sequential)
    assert isinstance(MeshFeaturizer(num_blocks=1, width=8, num_features=4, reconstructor_layers=-1).reconstructor, diffusion_net.layers.DiffusionNet)
    m = MeshFeaturizer(num_blocks=1, width=8)
    assert m.extractor_3d.C_in == 768 + 16 + 51 and m.reconstructor.out_features == 768


def test_neck_matches_the_reference():
    fx = lc.golden("fx_featurizer.npz")
    model, _ = lc.featurizer()
    verts = torch.from_numpy(fx["verts"].astype(np.float32))
    with torch.no_grad():
        pos = model.positional_encoding(verts * np.pi * 6)
        hks = diffusion_net.geometry.compute_hks_autoscale(torch.from_numpy(fx["evals"]), torch.from_numpy(fx["evecs"]), model.num_hks)
    assert pos.shape == (len(verts), 51) and hks.shape == (len(verts), 16)
    lc.check(pos, fx["pos_enc"], fx["floor_pos"], "positional_encoding")
    lc.check(hks, fx["hks"], fx["floor_hks"], "hks")


@pytest.mark.parametrize("given", [True, False])
def test_forward_matches_the_reference(given):
    fx = lc.golden("fx_featurizer.npz")
    model, _ = lc.featurizer()
    mesh, ops, cams, fts, p2f = lc.featurizer_inputs()
    with torch.no_grad():
        outn, out, mv = model(None, mesh, ops, cams, return_mvfeatures=True, fts=fts, pix2face=p2f if given else None, route="host")
        alone = model(None, mesh, ops, cams, fts=fts, route="host")
    assert model.extractor_3d.last_route == "torch"
    lc.check(mv, fx["mv_features"], fx["floor_mv"], "mv_features")
    lc.check(out, fx["out"], fx["f32_floor"], "out")
    lc.check(outn, fx["out_normalized"], fx["floor_normalized"], "out_normalized")
    assert torch.equal(alone, outn)


def test_refusals():
    model, _ = lc.featurizer()
    mesh, ops, cams, fts, _ = lc.featurizer_inputs()
    with pytest.raises(ValueError, match="fts"):
        model(None, mesh, ops, cams)
    with pytest.raises(ValueError, match="cameras"):
        model(None, mesh, ops, None, fts=fts)
    with pytest.raises(ValueError, match="route"):
        model(None, mesh, ops, cams, fts=fts, route="gpu")
    with pytest.raises(ValueError, match="fts"):
        model.forward_many([None], [mesh], None, [cams])
