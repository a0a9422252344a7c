"""CPU: PointRend (segmentron/models/pointrend.py) served by the overlay registry — registration,
config pruning, the reference's state_dict schema (tests/golden/pointrend_state_keys.json,
tools/gen_golden_pointrend.py), the optimizer quirk of a model without `encoder`, and the
drop-in: with the reference on sys.path, `segmentron.models.pointrend` (imported by the
reference's solver/loss.py:9) resolves to this repository."""
import json
import os

import pytest
import torch

from conftest import GOLDEN
from test_dropin import REF, _run, needs_ref

YAML = os.path.join(GOLDEN, "cityscapes_pointrend_deeplabv3_plus.yaml")


@pytest.fixture()
def pr_cfg():
    from segmentron_amd.config import cfg, reset_cfg
    reset_cfg()
    cfg.update_from_file(YAML)
    cfg.update_from_list(["TRAIN.BACKBONE_PRETRAINED", "False"])
    cfg.PHASE = "test"
    cfg.check_and_freeze()
    yield cfg
    reset_cfg()


def test_registered_and_config_subtrees_kept(pr_cfg):
    from segmentron_amd.models.model_zoo import MODEL_REGISTRY
    assert "PointRend" in MODEL_REGISTRY.get_list()
    assert pr_cfg.MODEL.POINTREND.BASEMODEL == "DeepLabV3_Plus"
    assert pr_cfg.MODEL.DEEPLABV3_PLUS.ENABLE_DECODER is False
    assert "DANET" not in pr_cfg.MODEL and "HRNET" not in pr_cfg.MODEL


def test_state_dict_schema_equals_reference(pr_cfg):
    import segmentron_amd
    ref = json.load(open(os.path.join(GOLDEN, "pointrend_state_keys.json")))
    model = segmentron_amd.get_segmentation_model()
    got = [(k, list(v.shape)) for k, v in model.state_dict().items()]
    assert got == [(k, list(s)) for k, s in ref["keys"]]
    assert sum(p.numel() for p in model.parameters()) == ref["n_params"]
    assert (model.encoder is None) == ref["encoder_is_none"] is True
    # the MLP's K = 275 stays unpadded in the parameter (padding lives in the packed copy only)
    assert tuple(model.head.mlp[0].weight.shape) == (256, 275, 1)


def test_optimizer_single_group_and_default_bn_eps(pr_cfg):
    """solver/optimizer.py:16,31-34: no `encoder` -> one parameter group at SOLVER.LR, and
    BN_EPS_FOR_ENCODER (1e-3 in the yaml) is not applied."""
    import segmentron_amd
    from segmentron_amd.solver.optimizer import get_optimizer
    assert pr_cfg.MODEL.BN_EPS_FOR_ENCODER == 1e-3
    model = segmentron_amd.get_segmentation_model()
    opt = get_optimizer(model)
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["lr"] == pr_cfg.SOLVER.LR
    eps = {m.eps for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)}
    assert eps == {1e-5}


def test_public_functions_need_the_device():
    from segmentron_amd.models.pointrend import point_sample, sampling_points
    x = torch.zeros(1, 19, 5, 7)
    with pytest.raises(RuntimeError):
        point_sample(x, torch.rand(1, 4, 2), align_corners=False)
    with pytest.raises(RuntimeError):
        sampling_points(x, 4, training=False)
    with pytest.raises(NotImplementedError):
        point_sample(x, torch.rand(1, 4, 2), align_corners=True)


def test_lazy_outputs_dispatch_without_materialising():
    """CoarseLogits keeps F.interpolate pending (a LogitsView of the same low-resolution tensor
    whose fused loss also takes x16, while LogitsView's own limit stays 8.1x); PointLogits reports the reference's [N, nclass, P] and exposes its tensor to DDP."""
    import dataclasses
    import torch.nn.functional as TF
    from segmentron_amd import functional as F
    from segmentron_amd.models.pointrend import CoarseLogits, CoarseUpsampled, PointLogits
    lo = torch.zeros(2, 5, 7, 24)[..., :19]
    c = CoarseLogits(lo, (5, 7))
    assert c.shape == (2, 19, 5, 7)
    up = TF.interpolate(c, (65, 97), mode="bilinear", align_corners=True)
    assert type(up) is CoarseUpsampled and isinstance(up, F.LogitsView)
    assert up.lo is lo and up.out_hw == (65, 97) and up.align_corners
    t = torch.zeros(2, 65, 97, dtype=torch.long)
    args = (t, None, None, -1, None, "mean", 0.0)
    assert up._fusable(*args)  # 16x
    assert not F.LogitsView(lo, (65, 97))._fusable(*args)  # other models: unchanged 8.1x limit
    t2 = torch.zeros(2, 69, 97, dtype=torch.long)
    assert not CoarseUpsampled(lo, (69, 97))._fusable(t2, *args[1:])  # 17x
    rows = torch.zeros(1, 1, 2 * 64, 20)[..., :19]
    r = PointLogits(rows, 2)
    assert r.shape == (2, 19, 64) and r.dim() == 3 and len(r) == 2
    assert any(f.name == "lo" for f in dataclasses.fields(r))
    assert r._full is None


@needs_ref
def test_reference_loss_binds_to_our_point_sample_and_trainer_builds(tmp_path):
    """The reference's tools/train.py import block, then its Trainer on the PointRend yaml: the
    model is ours, the criterion the reference's PointRendLoss, and solver/loss.py's
    `point_sample` is this repository's."""
    import numpy as np
    from PIL import Image
    rng = np.random.RandomState(0)
    for split, n in (("train", 2), ("val", 2)):
        for i in range(n):
            d_img = tmp_path / "datasets" / "cityscapes" / "leftImg8bit" / split / "aachen"
            d_gt = tmp_path / "datasets" / "cityscapes" / "gtFine" / split / "aachen"
            d_img.mkdir(parents=True, exist_ok=True)
            d_gt.mkdir(parents=True, exist_ok=True)
            Image.fromarray(rng.randint(0, 255, (96, 192, 3), dtype=np.uint8)).save(
                d_img / ("aachen_%06d_000019_leftImg8bit.png" % i))
            Image.fromarray(rng.randint(0, 34, (96, 192), dtype=np.uint8)).save(
                d_gt / ("aachen_%06d_000019_gtFine_labelIds.png" % i))
    # tools/launch.py adds the torchvision / thop stand-ins when find_spec() misses them; earlier
    # tests of the session may have put the oracle's in-memory stubs into sys.modules
    import importlib.machinery
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shims = os.path.join(root, "segmentron_amd", "shims")
    search = [p for p in sys.path if os.path.abspath(p or ".") != shims]
    paths = [root]
    if any(importlib.machinery.PathFinder.find_spec(n, search) is None
           for n in ("torchvision", "thop")):
        paths.append(shims)
    out = _run("""
        import importlib.util, os, sys, types
        ref, root = sys.argv[1], sys.argv[2]
        script = os.path.join(ref, 'tools', 'train.py')
        sys.argv = [script]
        spec = importlib.util.spec_from_file_location('ref_tools_train', script)
        train = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(train)
        import segmentron, segmentron_amd
        import segmentron.solver.loss as L
        mod = sys.modules['segmentron.models.pointrend']
        assert mod.__file__.startswith(os.path.dirname(segmentron_amd.__file__)), mod.__file__
        assert L.point_sample is segmentron_amd.models.pointrend.point_sample
        cfg = train.cfg
        cfg.update_from_file(os.path.join(ref, 'configs', 'cityscapes_pointrend_deeplabv3_plus.yaml'))
        cfg.update_from_list(['TRAIN.BATCH_SIZE', '2', 'TRAIN.CROP_SIZE', '64', 'TRAIN.BASE_SIZE',
                              '96', 'DATASET.WORKERS', '0', 'TRAIN.BACKBONE_PRETRAINED', 'False',
                              'TRAIN.LOG_SAVE_DIR', os.path.join(root, 'log'), 'TRAIN.EPOCHS', '1'])
        cfg.PHASE = 'train'
        cfg.ROOT_PATH = root
        cfg.check_and_freeze()
        args = types.SimpleNamespace(no_cuda=True, local_rank=0, resume=None, log_iter=10,
                                     val_epoch=1, skip_val=True, config_file='x', opts=[])
        train.default_setup(args)
        trainer = train.Trainer(args)
        assert type(trainer.model).__module__ == 'segmentron_amd.models.pointrend'
        assert type(trainer.model).__name__ == 'PointRend'
        assert type(trainer.criterion).__name__ == 'PointRendLoss'
        assert len(trainer.optimizer.param_groups) == 1
        print('POINTREND_OK')
    """, env_extra={"PYTHONPATH": os.pathsep.join(paths)}, args=[REF, str(tmp_path)])
    assert "POINTREND_OK" in out


def test_oracle_reproduces_the_reference_run():
    """The test-side restatement (tests/_pointrend_oracle.py) that the GPU tests compare against
    reproduces the reference's own PointRend + PointRendLoss (tests/golden/pointrend_ref_run.npz:
    recorded torch.rand draws, synthesised weights): the points, the loss and the evaluation
    output."""
    import numpy as np
    import _pointrend_oracle as O
    from oracle import synth
    g = np.load(os.path.join(GOLDEN, "pointrend_ref_run.npz"))
    keys = json.load(open(os.path.join(GOLDEN, "pointrend_state_keys.json")))["keys"]
    sd = O.state([(k, tuple(s)) for k, s in keys])
    over, cover = O.draws()
    assert torch.equal(over, torch.from_numpy(g["over"]))
    assert torch.equal(cover, torch.from_numpy(g["cover"]))
    x = synth.synth_images(O.B, O.H, O.W, seed=1)
    y = synth.synth_targets(O.B, O.H, O.W, seed=1)
    loss, _, _, _, _, pts = O.train(sd, x, y, torch.float32, over, cover)
    assert torch.equal(pts, torch.from_numpy(g["points"]))
    assert abs(loss - float(g["loss"])) <= 1e-5 * float(g["loss"])
    steps = []
    fine = O.evaluate(sd, x, steps)
    assert steps == [(14, 18), (28, 36), (56, 72), (O.H, O.W)]
    ref = torch.from_numpy(g["fine_sub2"])
    assert (fine[..., ::2, ::2] - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()


def test_graph_mode_leaves_pointrend_eager_and_logs_once(pr_cfg, monkeypatch, caplog):
    """SEGMENTRON_HIP_GRAPH=1: PointRend is not captured (data-dependent points), the log line
    appears once per process; other models still get their TransparentTrainGraph."""
    import logging
    import segmentron_amd
    from segmentron_amd.models import model_zoo
    monkeypatch.setenv("SEGMENTRON_HIP_GRAPH", "1")
    monkeypatch.setattr(model_zoo, "_EAGER_NOTED", set())
    with caplog.at_level(logging.INFO):
        a = segmentron_amd.get_segmentation_model()
        b = segmentron_amd.get_segmentation_model()
    assert "_transparent_graph" not in a.__dict__ and "_transparent_graph" not in b.__dict__
    assert sum("PointRend is not graph-captured" in r.getMessage() for r in caplog.records) == 1
    from segmentron_amd.config import cfg, reset_cfg
    from conftest import C3_OVERRIDES
    reset_cfg()
    cfg.update_from_list(C3_OVERRIDES)
    cfg.PHASE = "test"
    cfg.check_and_freeze()
    m = segmentron_amd.get_segmentation_model()
    assert "_transparent_graph" in m.__dict__
    m._transparent_graph.uninstall()
