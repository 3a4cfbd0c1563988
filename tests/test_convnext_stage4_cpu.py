"""ConvNeXtExtractor(n_stages=4) on the module side (CPU): construction for ConvNeXt-T / -S, the state-dict layout of torchvision's
features[0:8] re-indexed as the reference's `stages`, and the refusal of n_stages outside 1..4 (reference models/feature_pyramid.py:28-54)."""
import pytest


@pytest.mark.parametrize("model,depth3", [("tiny", 9), ("small", 27)])
def test_four_stage_extractor_constructs_with_torchvision_layout(model, depth3):
    from gecco_amd.models.feature_pyramid import ConvNeXtExtractor
    m = ConvNeXtExtractor(n_stages=4, model=model, pretrained=False)
    assert len(m.stages) == 4
    sd = m.state_dict()
    assert sd["stages.0.0.0.weight"].shape == (96, 3, 4, 4) and sd["stages.0.0.1.weight"].shape == (96,)
    assert sd["stages.3.0.0.weight"].shape == (384,) and sd["stages.3.0.1.weight"].shape == (768, 384, 2, 2)
    assert sd["stages.3.1.0.block.0.weight"].shape == (768, 1, 7, 7) and sd["stages.3.1.0.block.2.weight"].shape == (768,)
    assert sd["stages.3.1.2.block.3.weight"].shape == (3072, 768) and sd["stages.3.1.2.block.5.weight"].shape == (768, 3072)
    assert sd["stages.3.1.2.layer_scale"].shape == (768, 1, 1) and "stages.3.1.3.layer_scale" not in sd
    assert f"stages.2.1.{depth3 - 1}.layer_scale" in sd and f"stages.2.1.{depth3}.layer_scale" not in sd
    # torchvision's features.{2s}.* / features.{2s+1}.* are stages.{s}.0.* / stages.{s}.1.* (the pretrained=True mapping)
    tv_indices = {2 * int(k.split(".")[1]) + int(k.split(".")[2]) for k in sd}
    assert tv_indices == set(range(8))
    # the fourth stage: downsample (LayerNorm 384 + Conv 384 -> 768, k2 s2) + 3 CNBlocks of 768
    n4 = sum(v.numel() for k, v in sd.items() if k.startswith("stages.3."))
    assert n4 == (2 * 384 + 768 * 384 * 4 + 768) + 3 * (768 * 49 + 768 + 2 * 768 + 768 * 3072 + 3072 + 3072 * 768 + 768 + 768), n4
    three = ConvNeXtExtractor(n_stages=3, model=model, pretrained=False).state_dict()
    assert {k: v.shape for k, v in three.items()} == {k: v.shape for k, v in sd.items() if not k.startswith("stages.3.")}


@pytest.mark.parametrize("n", [0, 5])
def test_n_stages_outside_one_to_four_raises(n):
    from gecco_amd.models.feature_pyramid import ConvNeXtExtractor
    with pytest.raises(ValueError):
        ConvNeXtExtractor(n_stages=n, model="tiny", pretrained=False)


def test_four_level_conditional_model_state_dict():
    """RayNetwork(context_dims=(96, 192, 384, 768)): GroupNormBNC(16) over 1440 channels (90 per group), img_feature_proj 1440 -> d."""
    from tests.test_modules_cpu import build_cond
    from gecco_amd.models.feature_pyramid import ConvNeXtExtractor
    m = build_cond(128, 1, (96, 192, 384, 768), conditioner=ConvNeXtExtractor(n_stages=4, model="tiny", pretrained=False))
    net = m.backbone.model
    assert net.img_feature_proj[0].num_channels == 1440 and net.img_feature_proj[0].num_groups == 16
    assert m.state_dict()["backbone.model.img_feature_proj.1.weight"].shape == (128, 1440)
    assert any(k.startswith("conditioner.stages.3.") for k in m.state_dict())


@pytest.mark.parametrize("n,hw,maps", [(4, (137, 137), [(34, 34), (17, 17), (8, 8), (4, 4)]),
                                       (4, (201, 143), [(50, 35), (25, 17), (12, 8), (6, 4)]),
                                       (4, (33, 33), [(8, 8), (4, 4), (2, 2), (1, 1)]), (3, (130, 150), [(32, 37), (16, 18), (8, 9)])])
def test_map_sizes_floor_like_torchvision(n, hw, maps):
    """Any image size: the stem and every downsample floor like torchvision's strided Conv2d (the reference's ShapeNet images are
    137 x 137, data/shapenet_cond.py)."""
    import torch
    import torch.nn.functional as F
    from gecco_amd.models.feature_pyramid import ConvNeXtExtractor
    m = ConvNeXtExtractor(n_stages=n, model="tiny", pretrained=False)
    assert m.map_sizes(*hw) == maps
    x = F.conv2d(torch.zeros(1, 3, *hw), torch.zeros(1, 3, 4, 4), stride=4)
    sizes = [tuple(x.shape[2:])]
    for _ in range(n - 1):
        x = F.conv2d(x, torch.zeros(1, 1, 2, 2), stride=2)
        sizes.append(tuple(x.shape[2:]))
    assert sizes == maps
    m.check_image_size(*hw)


@pytest.mark.parametrize("n,hw", [(4, (20, 20)), (4, (64, 31)), (3, (15, 64)), (1, (3, 40))])
def test_too_small_image_is_refused_before_any_launch(n, hw):
    """An image whose pyramid would have an empty map is refused by the module, before it reaches a kernel (CPU tensors: the
    refusal comes before the device is touched)."""
    import torch
    from gecco_amd.models.feature_pyramid import ConvNeXtExtractor
    from gecco_amd.structs import Context3d
    m = ConvNeXtExtractor(n_stages=n, model="tiny", pretrained=False)
    ctx = Context3d(image=torch.rand(1, 3, *hw), K=torch.eye(3)[None])
    for grad in (False, True):
        with torch.set_grad_enabled(grad), pytest.raises(ValueError, match="empty"):
            m(ctx)
