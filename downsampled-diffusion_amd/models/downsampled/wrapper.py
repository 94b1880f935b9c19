"""Factories for the dDDPM resampling networks (reference models/downsampled/wrapper.py:6-59): all three values of
config['d_mode'] / config['u_mode'], chosen independently.
    'convolutional_res'  ConvResNet
    'convolutional'      SimpleDownConv / SimpleUpConv, called as the reference calls them: unet_in is their `dim`
    'deterministic'      Interpolate (bicubic, align_corners=True, no parameters)
"""
import numpy as np

from .convblocks import ConvResNet, Interpolate, SimpleDownConv, SimpleUpConv


def _common(config, shape):
    assert shape[1] == shape[2]
    assert shape[0] == 1 or shape[0] == 3
    return shape[0], config['d_chans'], config['unet_in'], config['d_dropout'], config['n_downsamples']


def _deterministic_channels(which, img_ch, lat_ch):
    if lat_ch != img_ch:
        raise ValueError(f"{which} = 'deterministic' is a bicubic resize and keeps the channel count: unet_in must equal the image's "
                         f"{img_ch} colour channels (got unet_in = {lat_ch})")


def get_upsampling(config: dict, shape: tuple):
    """latent (unet_in channels) -> image (shape[0] channels), wrapper.py:6-30"""
    img_ch, dim, lat_ch, dropout, n_down = _common(config, shape)
    mode = config['u_mode']
    if mode == 'deterministic':
        _deterministic_channels('u_mode', img_ch, lat_ch)
        return Interpolate((shape[1], shape[2]), img_ch)
    if mode == 'convolutional':
        return SimpleUpConv(lat_ch, img_ch, n_down)
    if mode == 'convolutional_res':
        return ConvResNet(dim, lat_ch, img_ch, n_down, upsample=True, dropout=dropout, n_blocks=config['u_n_blocks'])
    raise NotImplementedError(f'Upsampling method for "{mode}" not implemented!')


def get_downsampling(config: dict, shape: tuple):
    """image -> latent, wrapper.py:33-59"""
    img_ch, dim, lat_ch, dropout, n_down = _common(config, shape)
    mode = config['d_mode']
    if mode == 'deterministic':
        scale = np.power(2, n_down).astype(int)
        size = (int(shape[1] / scale), int(shape[2] / scale))
        assert size[0] % 2 == 0, 'result from downsampling should have even dimensions.'
        _deterministic_channels('d_mode', img_ch, lat_ch)
        return Interpolate(size, img_ch)
    if mode == 'convolutional':
        return SimpleDownConv(lat_ch, img_ch, n_down)
    if mode == 'convolutional_res':
        return ConvResNet(dim, img_ch, lat_ch, n_down, upsample=False, dropout=dropout, n_blocks=config['d_n_blocks'])
    raise NotImplementedError(f'Downsampling method for "{mode}" not implemented!')
