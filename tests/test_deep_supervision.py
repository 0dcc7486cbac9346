"""Deep supervision, host side: what the option registers on the networks (and what it leaves alone when it is off), the
per-level weights, the config keys, the inference loader's handling of the auxiliary heads, and the C-ABI table."""
import types
from collections import OrderedDict

import pytest
import torch

from conftest import golden_json

HEADS = (('ds_out_64', 64), ('ds_out_128', 128), ('ds_out_256', 256))


def _net(plugin, cin, ncls, **kw):
    import importlib
    return importlib.import_module('segmentation3d.network.' + plugin).SegmentationNet(cin, ncls, **kw)


@pytest.mark.parametrize('tag', ['vnet_1_2', 'vbnet_1_2', 'vnet_1_5', 'vbnet_1_5'])
def test_off_by_default_keeps_the_state_dict(tag):
    plugin, cin, ncls = tag.split('_')
    ref = [(k, tuple(s)) for k, s in golden_json('state_dict_shapes')[tag]['keys']]
    for kw in ({}, {'deep_supervision': 0}):
        net = _net(plugin, int(cin), int(ncls), **kw)
        assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == ref
        assert [k for k, _ in net.named_parameters()] == [k for k, _ in ref]
        assert not any(k.startswith('ds_out_') for k, _ in net.named_modules())


@pytest.mark.parametrize('plugin,ncls', [('vnet', 2), ('vbnet', 3)])
@pytest.mark.parametrize('levels', [1, 2, 3])
def test_heads_follow_out_block(plugin, ncls, levels):
    base = [(k, tuple(v.shape)) for k, v in _net(plugin, 1, ncls).state_dict().items()]
    got = [(k, tuple(v.shape)) for k, v in _net(plugin, 1, ncls, deep_supervision=levels).state_dict().items()]
    assert base[-1][0].startswith('out_block.')
    expect = []
    for name, cin in HEADS[:levels]:
        expect += [(name + '.conv.weight', (ncls, cin, 1, 1, 1)), (name + '.conv.bias', (ncls,))]
    assert got == base + expect


def test_initialisers_reach_the_heads():
    from segmentation3d.network import vnet
    net = vnet.SegmentationNet(1, 2, deep_supervision=2)
    for head in (net.ds_out_64, net.ds_out_128):
        head.conv.bias.data.fill_(1.0)
    vnet.parameters_kaiming_init(net)
    assert float(net.ds_out_64.conv.bias.detach().abs().max()) == 0.0
    assert float(net.ds_out_128.conv.bias.detach().abs().max()) == 0.0
    vnet.parameters_gaussian_init(net)
    assert float(net.ds_out_128.conv.weight.detach().std()) < 0.02


@pytest.mark.parametrize('bad', [-1, 4, 1.0, True, '2', None])
def test_invalid_level_count_raises(bad):
    with pytest.raises(ValueError):
        _net('vnet', 1, 2, deep_supervision=bad)


def test_forward_deep_needs_heads():
    net = _net('vnet', 1, 2)
    with pytest.raises(ValueError):
        net.forward_deep(torch.zeros(1, 1, 16, 16, 16))


def test_forward_deep_refuses_bf16_mode():
    from segmentation3d import _ops
    net = _net('vnet', 1, 2, deep_supervision=1)
    with _ops.activation_dtype('bf16'):
        with pytest.raises(ValueError, match='fp32'):
            net.forward_deep(torch.zeros(1, 1, 16, 16, 16))


def test_default_weights():
    from segmentation3d.loss.deep_supervision_loss import DeepSupervisionLoss, normalise_level_weights
    expect = {1: [2 / 3, 1 / 3], 2: [4 / 7, 2 / 7, 1 / 7], 3: [8 / 15, 4 / 15, 2 / 15, 1 / 15]}
    for levels, w in expect.items():
        assert normalise_level_weights(levels) == pytest.approx(w, rel=1e-15)
        assert DeepSupervisionLoss(torch.nn.Identity(), levels).weights == pytest.approx(w, rel=1e-15)
    assert normalise_level_weights(2, [2, 1, 1]) == pytest.approx([0.5, 0.25, 0.25])
    assert normalise_level_weights(1, (1, 0)) == [1.0, 0.0]


@pytest.mark.parametrize('levels,weights', [(0, None), (4, None), (-1, None), (1.0, None), (True, None), (2, [1, 1]),
                                            (2, [1, 1, 1, 1]), (2, [0, 1, 1]), (2, [1, -1, 1]), (1, [float('nan'), 1]),
                                            (1, [1, float('inf')]), (1, 'ab'), (1, 3)])
def test_invalid_levels_or_weights_raise(levels, weights):
    from segmentation3d.loss.deep_supervision_loss import DeepSupervisionLoss
    with pytest.raises(ValueError):
        DeepSupervisionLoss(torch.nn.Identity(), levels, weights)


def test_loss_checks_the_number_of_outputs():
    from segmentation3d.loss.deep_supervision_loss import DeepSupervisionLoss
    loss = DeepSupervisionLoss(torch.nn.Identity(), 2)
    with pytest.raises(ValueError):
        loss([torch.zeros(1, 2, 8, 8, 8)], torch.zeros(1, 1, 8, 8, 8))
    with pytest.raises(ValueError):
        loss(torch.zeros(1, 2, 8, 8, 8), torch.zeros(1, 1, 8, 8, 8))


def test_config_keys_default_when_absent():
    from segmentation3d.core.seg_train import deep_supervision_from_config
    assert deep_supervision_from_config(types.SimpleNamespace(epochs=1, batchsize=1)) == {
        'deep_supervision': 0, 'deep_supervision_weights': None}
    cfg = types.SimpleNamespace(deep_supervision=2, deep_supervision_weights=(4, 2, 1))
    assert deep_supervision_from_config(cfg) == {'deep_supervision': 2, 'deep_supervision_weights': [4, 2, 1]}


def test_shipped_config_keeps_the_reference_keys():
    import os
    from conftest import PKG
    text = open(os.path.join(PKG, 'segmentation3d', 'config', 'train_config.py')).read()
    assert 'deep_supervision' not in text


def test_train_step_signature_defaults():
    import inspect
    from segmentation3d.core.seg_train import TrainStep
    params = inspect.signature(TrainStep.__init__).parameters
    assert params['deep_supervision'].default == 0 and params['deep_supervision_weights'].default is None


def test_inference_loader_drops_the_heads():
    from segmentation3d.utils.model_io import inference_state_dict, strip_deep_supervision
    deep = _net('vnet', 1, 2, deep_supervision=3)
    plain = _net('vnet', 1, 2)
    state = OrderedDict(('module.' + k, v) for k, v in deep.state_dict().items())
    kept = inference_state_dict(state)
    assert list(kept) == list(plain.state_dict())
    plain.load_state_dict(kept)                       # strict: nothing missing, nothing unexpected
    for k, v in plain.state_dict().items():
        assert torch.equal(v, deep.state_dict()[k])
    untouched = plain.state_dict()
    assert strip_deep_supervision(untouched) is untouched
    deep.load_state_dict(deep.state_dict())           # a resume with the same deep_supervision takes every key


def test_checkpoint_state_records_the_level_count():
    from segmentation3d.utils.model_io import checkpoint_state
    cfg = types.SimpleNamespace(dataset=types.SimpleNamespace(spacing=[1, 1, 1], interpolation='LINEAR', num_classes=2,
                                                              crop_normalizers=[None]), net=types.SimpleNamespace(name='vnet'))
    assert checkpoint_state(_net('vnet', 1, 2, deep_supervision=2), 1, 2, cfg, 16, 1)['deep_supervision'] == 2
    state = checkpoint_state(_net('vnet', 1, 2), 1, 2, cfg, 16, 1)
    assert state['deep_supervision'] == 0 and state['in_channels'] == 1


def test_ctypes_table_holds_the_new_entries():
    from segmentation3d import _engine
    names = ('seg3d_ds_head_supported', 'seg3d_ds_head_fwd', 'seg3d_ds_head_bwd_workspace_floats', 'seg3d_ds_head_bwd',
             'seg3d_ds_head_bwd_finalize', 'seg3d_label_pyramid')
    assert set(names) <= set(_engine.symbols())
    assert _engine.lib().seg3d_abi_version() == 2
    # the size helpers are host arithmetic
    for cin, c, ok in ((64, 2, 1), (256, 8, 1), (4, 1, 1), (260, 2, 0), (66, 2, 0), (64, 9, 0), (64, 0, 0), (0, 2, 0)):
        assert _engine.query('seg3d_ds_head_supported', cin, c) == ok, (cin, c)
    n = _engine.query('seg3d_ds_head_bwd_workspace_floats', 2, 105, 64, 2)
    assert n > 0 and n % (2 * 64 + 2) == 0
    assert _engine.query('seg3d_ds_head_bwd_workspace_floats', 2, 105, 66, 2) == 0
