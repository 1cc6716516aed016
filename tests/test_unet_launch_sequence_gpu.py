"""The launches of the ray-drop U-Net, in order (lidarnerf/unet.py, lidarnerf/unet_train.py): the entry points RayDropUNet.forward,
predict_mask, train_forward and train_backward call on the smallest image the training layer accepts, 1 x 10 x 16 x 32 (1 x 16 x 16
leaves one value per channel at the deepest level, which batch statistics refuse).  The lists are written out as observed when each
walk still spelled its layer numbers out by hand, so a change of the layer table that reorders, drops or adds a launch shows here
by name."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CONV, UP = "lnh_unet_conv3x3", "lnh_unet_upconv2x2"
FORWARD = ["lnh_unet_input",
           CONV, CONV,                                      # inc
           CONV, CONV, CONV, CONV, CONV, CONV, CONV, CONV,  # down1 .. down4
           UP, CONV, CONV, UP, CONV, CONV, UP, CONV, CONV, UP, CONV, CONV,  # up1 .. up4
           "lnh_unet_head"]

LAYER = ["lnh_unet_pack_conv3x3", "lnh_unet_conv3x3_raw", "lnh_unet_bn_stats", "lnh_unet_bn_relu"]
UP_BLOCK = ["lnh_unet_pack_upconv", UP] + LAYER + LAYER
TRAIN_FORWARD = ["lnh_unet_input"] + LAYER + LAYER + (LAYER + LAYER) * 4 + UP_BLOCK + UP_BLOCK + UP_BLOCK + UP_BLOCK + ["lnh_unet_head"]

BN, WG, DX = "lnh_unet_bn_relu_backward", "lnh_unet_conv3x3_backward_weight", "lnh_unet_conv3x3_raw"
UPW, UPD, POOL = "lnh_unet_upconv2x2_backward_weight", "lnh_unet_upconv2x2_backward_data", "lnh_unet_pool_backward"
TRAIN_BACKWARD = ["lnh_unet_head_backward",
                  BN, DX, BN, DX, UPW, UPD,  # up4: layers 17, 16
                  BN, DX, BN, DX, UPW, UPD,  # up3
                  BN, DX, BN, DX, UPW, UPD,  # up2
                  BN, DX, BN, DX, UPW, UPD,  # up1: layers 11, 10
                  BN, DX, BN, DX, POOL,      # down4: layers 9, 8
                  BN, DX, BN, DX, POOL,      # down3
                  BN, DX, BN, DX, POOL,      # down2
                  BN, DX, BN, DX, POOL,      # down1: layers 3, 2
                  BN, DX, BN]                # inc: layer 0 has no data gradient
TRAIN_BACKWARD_CONV_WEIGHTS = ["lnh_unet_head_backward",
                               BN, WG, DX, BN, WG, DX, UPW, UPD,
                               BN, WG, DX, BN, WG, DX, UPW, UPD,
                               BN, WG, DX, BN, WG, DX, UPW, UPD,
                               BN, WG, DX, BN, WG, DX, UPW, UPD,
                               BN, WG, DX, BN, WG, DX, POOL,
                               BN, WG, DX, BN, WG, DX, POOL,
                               BN, WG, DX, BN, WG, DX, POOL,
                               BN, WG, DX, BN, WG, DX, POOL,
                               BN, WG, DX, BN, WG]


def test_launch_sequences(monkeypatch):
    from lidarnerf import _hip
    from lidarnerf import unet_train as ut
    from lidarnerf.unet import RayDropUNet
    torch.manual_seed(0)
    net = RayDropUNet().cuda()
    x = torch.randn(1, 10, 16, 32, device="cuda")
    names, call = [], _hip.call

    def recorder(name, *args, **kwargs):
        names.append(name)
        return call(name, *args, **kwargs)

    monkeypatch.setattr(_hip, "call", recorder)

    def launches(fn):
        del names[:]
        out = fn()
        return list(names), out

    got, _ = launches(lambda: net(x))
    assert got == FORWARD and len(got) == 24
    got, _ = launches(lambda: net.predict_mask(x))
    assert got == FORWARD
    got, (logits, state) = launches(lambda: ut.train_forward(net, x))
    assert got == TRAIN_FORWARD and len(got) == 1 + 18 * 4 + 4 * 2 + 1
    d = torch.full_like(logits, 1e-3)
    got, grads = launches(lambda: ut.train_backward(net, state, d))
    assert got == TRAIN_BACKWARD and len(got) == 1 + 18 + 17 + 4 * 2 + 4 and len(grads) == 46
    got, grads = launches(lambda: ut.train_backward(net, state, d, conv_weights=True))
    assert got == TRAIN_BACKWARD_CONV_WEIGHTS and len(got) == len(TRAIN_BACKWARD) + 18 and len(grads) == 64
    torch.cuda.synchronize()
