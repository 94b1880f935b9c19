"""Which form -- tuned kernels with gradient hand-offs, or generic kernels on the padded pitch -- every module of the UNet takes in
training (ddk/forms.py: the one place that decides; trainers/autograd_unet.py walks by it).  The tables below are written out from
the rules the two former walks followed: a model whose unet_chan is no multiple of 32 ran EVERY module generic and handed no gradient
over; in the others a ResnetBlock followed gn_tuned of its output width, an attention block ln_tuned of its width, and every
Downsample carried its skip tensor's gradient.  No GPU: `Unet` is only constructed."""
import pytest

from ddk.forms import attention_tuned, gn_tuned, ln_tuned, pitch_tuned, resnet_tuned, training_forms
from models import Unet


def forms_of(chan, dims, cin=3):
    return training_forms(Unet(dict(unet_chan=chan, unet_in=cin, unet_dims=dims, unet_dropout=0.0)))


def of_kind(forms, *kinds):
    return [(f.c_out, f.tuned) for f in forms if f.kind in kinds]


def test_gn_tuned_takes_4_8_16_32_channels_per_group():
    assert all(gn_tuned(c, 8) for c in (32, 64, 128, 256))
    assert not any(gn_tuned(c, 8) for c in (96, 160, 192, 384, 512))
    assert not any(gn_tuned(c, 8) for c in (8, 16, 24, 40, 72, 200))          # 1, 2, 3, 5, 9, 25 channels per group
    assert gn_tuned(64, 4) and not gn_tuned(256, 4) and not gn_tuned(36, 8)


def test_ln_tuned_is_true_exactly_at_the_instantiated_widths():
    assert [c for c in range(8, 1025, 8) if ln_tuned(c)] == [32, 64, 128, 256, 512]


def test_a_padded_pitch_model_overrides_every_width():
    for c in (32, 64, 128, 256):
        assert resnet_tuned(32, c) and resnet_tuned(96, c) and attention_tuned(160, c)
        for dim in (8, 16, 24, 40, 72, 200):
            assert not pitch_tuned(dim) and not resnet_tuned(dim, c) and not attention_tuned(dim, c)
    assert pitch_tuned(32) and pitch_tuned(96) and not resnet_tuned(96, 96) and not attention_tuned(96, 96)


def test_forms_alternate_at_levels_of_32_64_96_128():
    forms = forms_of(32, (1, 2, 3, 4))
    T, G = True, False
    assert of_kind(forms, "resnet", "block") == [
        (32, T), (32, T), (64, T), (64, T), (96, G), (96, G), (128, T), (128, T),          # down
        (128, T), (128, T),                                                                # mid
        (96, G), (96, G), (64, T), (64, T), (32, T), (32, T),                              # up
        (32, T)]                                                                           # the final Block
    assert forms[-2].kind == "block" and forms[-2].name == "final_conv.0"
    assert of_kind(forms, "attention") == [(32, T), (64, T), (96, G), (128, T), (128, T), (96, G), (64, T), (32, T)]
    assert of_kind(forms, "down") == [(32, T), (64, T), (96, T)]          # a carry on the three levels with a Downsample
    assert of_kind(forms, "up") == [(96, T), (64, T), (32, T)]
    assert of_kind(forms, "out") == [(3, T)]


def test_forms_come_in_forward_order_with_the_modules_themselves():
    u = Unet(dict(unet_chan=32, unet_in=3, unet_dims=(1, 2, 3, 4), unet_dropout=0.0))
    forms = training_forms(u)
    names = dict(u.named_modules())
    assert all(names[f.name] is f.module for f in forms)
    want = []
    for i in range(4):
        want += [f"downs.{i}.{k}" for k in range(4 if i < 3 else 3)]
    want += ["mid_block1", "mid_attn", "mid_block2"]
    for i in range(3):
        want += [f"ups.{i}.{k}" for k in range(4)]
    want += ["final_conv.0", "final_conv.1"]
    assert [f.name for f in forms] == want


def test_groupnorm_generic_and_layernorm_tuned_at_512():
    forms = forms_of(128, (1, 4))
    T, G = True, False
    assert of_kind(forms, "resnet", "block") == [(128, T), (128, T), (512, G), (512, G), (512, G), (512, G), (128, T), (128, T), (128, T)]
    assert of_kind(forms, "attention") == [(128, T), (512, T), (512, T), (128, T)]
    assert of_kind(forms, "down") == [(128, T)]


@pytest.mark.parametrize("chan,dims,widths", [(16, (1, 2, 4, 8), (16, 32, 64, 128)), (24, (1, 2, 2, 2), (24, 48, 48, 48))])
def test_every_module_of_a_padded_pitch_model_is_generic(chan, dims, widths):
    """... and there is no carry, although 32, 64 and 128 pass gn_tuned and ln_tuned"""
    forms = forms_of(chan, dims)
    assert not any(f.tuned for f in forms)
    a, b, c, d = widths
    assert [f.c_out for f in forms if f.kind == "resnet"] == [a, a, b, b, c, c, d, d, d, d, c, c, b, b, a, a]
    assert [f.c_out for f in forms if f.kind == "attention"] == [a, b, c, d, d, c, b, a]
    assert [f.c_out for f in forms if f.kind == "down"] == [a, b, c] and [f.c_out for f in forms if f.kind == "up"] == [c, b, a]
    assert of_kind(forms, "block") == [(chan, False)] and of_kind(forms, "out") == [(3, False)]
