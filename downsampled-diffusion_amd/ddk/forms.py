"""Tuned or generic: which form of the training kernels a module of the UNet runs.  The one place that decides.

tuned   -- kernels instantiated for the width; gradients that meet at a tensor are handed from Function to Function (GradHandoff,
           SlabLink of ddk/autograd.py) and added in a conv / normalisation epilogue; the parameters as they are.
generic -- kernels that take the channel count at run time, on a pitch of pad32(C); zero-padded copies of every parameter
           (autograd.pad_param); autograd adds where two gradients meet.  Correct and complete, untuned.
Both ends of a hand-off follow the module that owns it, so a module is one or the other as a whole.
"""
from collections import namedtuple


def gn_tuned(c, groups=8):
    """the tuned training GroupNorm (gn_train_launch: a float4 unit count per pixel row that is a power of two <= 8) takes 4, 8, 16 or
    32 channels per group -- 32, 64, 128, 256 channels at 8 groups.  Every other width that is a multiple of 32 (96, 160, 192, 224,
    320, 384, 512, ...) runs the generic training kernels with pitch == C (GNMishGenericFn: C / groups <= 256)."""
    return c % groups == 0 and c // groups in (4, 8, 16, 32)


def ln_tuned(c):
    """the widths ddk_chan_layernorm_bwd has an instantiation for; the others run chan_layernorm_generic_bwd with pitch == C (C <= 512)"""
    return c in (32, 64, 128, 256, 512)


def pitch_tuned(dim):
    """a model of unet_chan = dim keeps every tensor at pitch == C.  Its Downsample / Upsample / final 1x1 convs then run on their own
    parameters and a Downsample carries the up path's gradient of its level's skip tensor.  In any other model (24, 40, ...) EVERY
    module is generic and no gradient is handed over -- also at levels whose width gn_tuned / ln_tuned would take (unet_chan = 16:
    levels of 32, 64, 128)."""
    return dim % 32 == 0


def resnet_tuned(dim, c_out, groups=8):
    """a ResnetBlock, or the final Block, of c_out channels in a model of unet_chan = dim"""
    return pitch_tuned(dim) and gn_tuned(c_out, groups)


def attention_tuned(dim, c):
    """a Residual(PreNorm(LinearAttention)) of c channels in a model of unet_chan = dim"""
    return pitch_tuned(dim) and ln_tuned(c)


# kind: "resnet" | "attention" | "down" | "up" | "block" (the final Block) | "out" (the final 1x1); c_out: the real channels it leaves
Form = namedtuple("Form", "name kind module c_out tuned")


def training_forms(unet):
    """The modules of a models.Unet that the training walk runs, in forward order, each with the form it takes.  Pure: reads widths only."""
    dim = unet.dim

    def resnet(name, rb):
        c = rb.block1.block[0].weight.shape[0]
        return Form(name, "resnet", rb, c, resnet_tuned(dim, c, rb.block1.groups))

    def attention(name, res, c):
        return Form(name, "attention", res, c, attention_tuned(dim, c))

    forms = []
    for side, levels in (("downs", unet.downs), ("ups", unet.ups)):
        for i, (rb1, rb2, attn, resample) in enumerate(levels):
            forms += [resnet(f"{side}.{i}.0", rb1), resnet(f"{side}.{i}.1", rb2)]
            c = forms[-1].c_out
            forms.append(attention(f"{side}.{i}.2", attn, c))
            if hasattr(resample, "conv"):                     # the last down level has nn.Identity() here
                forms.append(Form(f"{side}.{i}.3", "down" if side == "downs" else "up", resample, c, pitch_tuned(dim)))
        if side == "downs":
            forms.append(resnet("mid_block1", unet.mid_block1))
            forms.append(attention("mid_attn", unet.mid_attn, forms[-1].c_out))
            forms.append(resnet("mid_block2", unet.mid_block2))
    block, out = unet.final_conv
    forms.append(Form("final_conv.0", "block", block, dim, resnet_tuned(dim, dim, block.groups)))
    forms.append(Form("final_conv.1", "out", out, out.weight.shape[0], pitch_tuned(dim)))
    return forms
