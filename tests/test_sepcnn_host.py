"""SeparableCNN without a GPU: the CPU restatement the GPU tests lean on reproduces the reference's numbers (fixture g20,
tools/make_goldens_r7.py), and the model's constructor / state dict are the reference's."""
import pytest
import torch

import sepcnn_cpu_ref as SR
from fdet_amd.models.SeparableCNN import SeparableCNN


def _redraw(g):
    x_u8 = torch.randint(0, 256, (2, 3, 480, 480), generator=torch.Generator().manual_seed(int(g["x_seed"])), dtype=torch.uint8)
    assert int(x_u8.long().sum()) == int(g["x_sum"]) and torch.equal(x_u8[:, :, ::97, ::89], g["x_probe"])
    return x_u8


def _close(got, ref, what, tol=1e-5):
    err = float((got.double() - ref.double()).abs().max())
    assert err <= tol * max(float(ref.abs().max()), 1e-30), (what, err)


def test_cpu_restatement_reproduces_the_fixture(golden):
    g = golden("g20_separablecnn_F16")
    P = {k[len("param/"):]: v for k, v in g.items() if k.startswith("param/")}
    masks = {k[len("mask/"):]: v for k, v in g.items() if k.startswith("mask/")}
    x = _redraw(g).float() / 255.0
    with torch.no_grad():
        _close(SR.forward(P, x), g["y_eval_default"], "y_eval_default")
        _close(SR.forward(P, x, head_pad=3), g["y_eval_pad3"], "y_eval_pad3")
    y_train, loss, grads, after = SR.train_step(P, x, g["y"], masks, head_pad=3)
    _close(y_train, g["y_train"], "y_train")
    _close(loss, g["loss"], "loss")
    for n in P:
        _close(grads[n], g["grad/" + n], "grad " + n)
        _close(after[n], g["param_after/" + n], "param_after " + n)


def test_constructor_asserts_divisibility_by_16():
    with pytest.raises(AssertionError):
        SeparableCNN(filters=16, input_shape=(3, 472, 472))


def test_state_dict_is_the_references(golden):
    g = golden("g20_separablecnn_F16")
    model = SeparableCNN(filters=16, input_shape=(3, 480, 480))
    sd = model.state_dict()
    names = [str(n) for n in g["names"]]
    assert list(sd.keys()) == names == SR.param_names(10)
    for n in names:
        assert tuple(sd[n].shape) == tuple(g["param/" + n].shape) == SR.param_shapes(16)[n], n
    assert sum(p.numel() for p in model.parameters()) == int(g["n_params"]) == 14261
    model.load_state_dict({n: g["param/" + n] for n in names}, strict=True)


def test_default_constructor_builds_with_a_10x10_head_on_16_patches():
    model = SeparableCNN(filters=16, input_shape=(3, 480, 480))
    assert model.num_of_patches == 16
    h0, lv = model._geometry().levels()
    assert h0 == 60 and lv == [(60, 2), (30, 2)] + [(15, 1)] * 8
    assert SeparableCNN(filters=16, input_shape=(3, 512, 512), output_kernel_size=1)._geometry().levels()[1][:3] == \
        [(64, 2), (32, 2), (16, 1)]


def test_torchscript_export_is_refused_on_every_route(tmp_path):
    """The model's own method, ModelMeta.to_torchscript (what trainer.fit calls) and train_model --save."""
    from fdet_amd._native import FdetError
    from fdet_amd.models import ModelMeta
    from fdet_amd import torchscript, train_model
    model = SeparableCNN(filters=16, input_shape=(3, 480, 480), output_padding=3)
    for export in (model.to_torchscript, ModelMeta(model=model, log_path=tmp_path / "out.log").to_torchscript,
                   lambda p: torchscript.to_torchscript(model, p)):
        with pytest.raises(FdetError, match="TorchScript export is not built for SeparableCNN"):
            export(str(tmp_path / "m.pt"))
    assert not (tmp_path / "m.pt").exists()
    with pytest.raises(SystemExit):                      # refused while parsing, before any training
        train_model.main(["--model", "separablecnn", "--save", str(tmp_path / "m.pt"), "--epochs", "1"])


def test_coherent_head_picks_the_16x16_grid_or_refuses():
    from fdet_amd._native import FdetError
    assert SeparableCNN.coherent_head(480) == {"output_kernel_size": 6, "output_padding": 3}
    assert SeparableCNN.coherent_head(512) == {"output_kernel_size": 1, "output_padding": 0}
    for size in (480, 512):
        m = SeparableCNN(filters=16, input_shape=(3, size, size), **SeparableCNN.coherent_head(size))
        geo = m._geometry()
        last = geo.levels()[1][-1]
        assert last[0] // last[1] + 2 * geo.head_p - geo.head_k + 1 == m.num_of_patches == 16
    for size in (448, 496, 640):                         # last maps of 14, 31 and 10: no head of the model gives 16x16
        with pytest.raises(FdetError):
            SeparableCNN.coherent_head(size)
