"""Host-side behaviour of the ray-drop U-Net's entry points that needs no device: the argument checks of every lnh_unet_* entry
point and the answers of every *_workspace_size function.  One table of calls, used twice: by tests/golden/make_unet_host.py, which
records what a library answers into tests/golden/unet_host.json, and by tests/test_unet_cpu.py, which compares the library under
test with that record.  Every call of an entry point here is REFUSED (the record holds LNH_ERR_INVALID_ARG for each one, and the
test asserts that before it calls anything), so no call reaches a launch and the pointers are never dereferenced."""
P = 1 << 20  # any non-null 16-byte aligned address
OFF8, OFF4 = P + 8, P + 4  # aligned to 8 / 4 bytes only
BIG = 1 << 40  # a workspace size that is always enough
INVALID_ARG = -1
CHANNELS = (64, 128, 256, 512, 1024)
SHAPES = ((2, 23, 37), (1, 16, 16), (1, 66, 1030))  # the shapes of the CPU tests of the layouts

# entry point -> its arguments in order, as a call that passes every check (never made as it stands)
BASES = {
    "lnh_unet_input": dict(inp=P, N=1, C=10, H=16, W=16, out=P),
    "lnh_unet_conv3x3": dict(src0=P, C0=64, H0=16, W0=16, pool=0, src1=None, C1=0, H1=0, W1=0, weight=P, scale=P, shift=P, N=1, Cout=64,
                             tile=0, out=P),
    "lnh_unet_conv3x3_raw": dict(src0=P, C0=64, H0=16, W0=16, pool=0, src1=None, C1=0, H1=0, W1=0, weight=P, N=1, Cout=64, tile=0, out=P),
    "lnh_unet_upconv2x2": dict(inp=P, N=1, H=8, W=8, Cin=128, weight=P, bias=P, Cout=64, out=P),
    "lnh_unet_head": dict(inp=P, N=1, H=16, W=16, weight=P, bias=P, logits=P, mask=None),
    "lnh_unet_pool_backward": dict(x=P, N=1, H0=16, W0=16, C=64, dpool=P, dskip=None, skip_stride=0, dx=P),
    "lnh_unet_head_backward": dict(a=P, N=1, H=16, W=16, weight=P, dlogits=P, ws=P, ws_bytes=BIG, dx=P, dweight=P, dbias=P),
    "lnh_unet_pack_upconv": dict(weight=P, Cin=128, Cout=64, fwd=P, bwd=P),
    "lnh_unet_upconv2x2_backward_data": dict(dy=P, Hd=16, Wd=16, dy_stride=128, dy_offset=64, N=1, H=8, W=8, Cin=128, Cout=64, weight=P,
                                             dx=P),
    "lnh_unet_upconv2x2_backward_weight": dict(x=P, dy=P, Hd=16, Wd=16, dy_stride=128, dy_offset=64, N=1, H=8, W=8, Cin=128, Cout=64,
                                               ws=P, ws_bytes=BIG, dweight=P, dbias=P),
    "lnh_unet_pack_conv3x3": dict(weight=P, Cout=64, Cin=64, fwd=P, bwd=P),
    "lnh_unet_bn_stats": dict(z=P, M=256, C=64, gamma=P, beta=P, eps=1e-5, momentum=0.1, ws=P, ws_bytes=BIG, mean=P, invstd=P, scale=P,
                              shift=P, running_mean=None, running_var=None),
    "lnh_unet_bn_relu": dict(z=P, M=256, C=64, scale=P, shift=P, a=P),
    "lnh_unet_bn_relu_backward": dict(z=P, a=P, da=P, M=256, C=64, mean=P, invstd=P, scale=P, ws=P, ws_bytes=BIG, dz=P, dgamma=P, dbeta=P),
    "lnh_unet_conv3x3_backward_weight": dict(src0=P, C0=64, H0=16, W0=16, pool=0, src1=None, C1=0, H1=0, W1=0, dz=P, N=1, Cout=64, Cin=64,
                                             variant=0, ws=P, ws_bytes=BIG, dweight=P),
    "lnh_unet_loss_grad": dict(logits=P, masks=P, mask_dtype=0, M=256, loss_scale=1.0, ws=P, ws_bytes=BIG, loss=P, dlogits=P),
    "lnh_unet_grad_sumsq": dict(table=P, n=64, ws=P, ws_bytes=BIG, state=P),
    "lnh_unet_rmsprop_step": dict(table=P, n=64, state=P, loss_scale=1.0, max_norm=1.0, alpha=0.99, eps=1e-8, weight_decay=0.0,
                                  momentum=0.0),
}

_CAT = dict(src1=P, C1=64, H1=16, W1=16)  # a second source that fits the base of the 3 x 3 entry points
# what both 3 x 3 forward entry points and the weight gradient refuse alike (the names of the cases; a "+" joins two faults: which
# check speaks first)
_CONV_SHARED = {
    "null_src0": dict(src0=None), "pool2": dict(pool=2), "C0_0": dict(C0=0), "C0_48": dict(C0=48), "C0_2048": dict(C0=2048),
    "C1_48": dict(_CAT, C1=48), "C1_without_src1": dict(C1=64, H1=16, W1=16), "src1_without_C1": dict(src1=P),
    "Cout_0": dict(Cout=0), "Cout_96": dict(Cout=96), "Cout_2048": dict(Cout=2048),
    "N0": dict(N=0), "H0_0": dict(H0=0), "pooled_to_nothing": dict(pool=1, H0=1), "too_many_pixels": dict(N=2, H0=8192, W0=8192),
    "src1_taller": dict(_CAT, H1=17), "src1_two_narrower": dict(_CAT, W1=14), "src1_empty": dict(_CAT, H1=0),
    "src1_two_narrower_pooled": dict(_CAT, pool=1, H0=35, W0=35, H1=16, W1=15),
    "src0_misaligned": dict(src0=OFF8), "src1_misaligned": dict(_CAT, src1=OFF8),
    "null_src0+pool2": dict(src0=None, pool=2), "pool2+C0_48": dict(pool=2, C0=48), "C0_48+C1_48": dict(_CAT, C0=48, C1=48),
    "C1_48+without_src1": dict(C1=48), "src1_without_C1+Cout_96": dict(src1=P, Cout=96), "Cout_96+N0": dict(Cout=96, N=0),
    "N0+src1_taller": dict(_CAT, N=0, H1=17), "src1_taller+src0_misaligned": dict(_CAT, H1=17, src0=OFF8),
}
_CONV_FWD = dict(_CONV_SHARED, **{
    "null_weight": dict(weight=None), "null_out": dict(out=None), "weight_misaligned": dict(weight=OFF8), "out_misaligned": dict(out=OFF8),
    "tile3": dict(tile=3), "tile16": dict(tile=16), "src0_misaligned+tile3": dict(src0=OFF8, tile=3), "C0_32_C1_96": dict(_CAT, C0=32, C1=96, N=0),
})
_UP_BWD = {
    "null_dy": dict(dy=None), "Cin_32": dict(Cin=32), "Cin_96": dict(Cin=96), "Cin_2048": dict(Cin=2048), "Cout_0": dict(Cout=0),
    "Cout_2048": dict(Cout=2048), "N0": dict(N=0), "too_many_pixels": dict(H=4097, W=4096, Hd=8194, Wd=8192),
    "dy_shorter": dict(Hd=15), "dy_two_wider": dict(Wd=18), "dy_one_larger": dict(Hd=17, Wd=17, N=0),
    "stride_4": dict(dy_stride=132), "offset_4": dict(dy_offset=4), "stride_4096": dict(dy_stride=4096),
    "channels_past_stride": dict(dy_offset=72), "dy_misaligned": dict(dy=OFF8),
    "null_dy+Cin_96": dict(dy=None, Cin=96), "Cin_96+Cout_0": dict(Cin=96, Cout=0), "Cout_0+N0": dict(Cout=0, N=0),
    "N0+dy_shorter": dict(N=0, Hd=15), "dy_shorter+offset_4": dict(Hd=15, dy_offset=4), "offset_4+dy_misaligned": dict(dy_offset=4, dy=OFF8),
}
_BN = {"null_z": dict(z=None), "M1": dict(M=1), "M_over": dict(M=(1 << 26) + 1), "C0": dict(C=0), "C48": dict(C=48), "C2048": dict(C=2048),
       "workspace_too_small": dict(ws_bytes=16), "z_misaligned": dict(z=OFF8), "ws_misaligned": dict(ws=OFF8),
       "null_z+M1": dict(z=None, M=1), "M1+C48": dict(M=1, C=48), "C48+workspace_too_small": dict(C=48, ws_bytes=16),
       "workspace_too_small+z_misaligned": dict(ws_bytes=16, z=OFF8)}
_TABLE = {"null_table": dict(table=None), "null_state": dict(state=None), "n0": dict(n=0), "n65": dict(n=65), "table_misaligned": dict(table=OFF4),
          "state_misaligned": dict(state=OFF4), "null_table+n0": dict(table=None, n=0), "n65+state_misaligned": dict(n=65, state=OFF4)}
_INF, _NAN = float("inf"), float("nan")

# entry point -> {case: what differs from the base}
WRONG = {
    "lnh_unet_input": {"null_in": dict(inp=None), "null_out": dict(out=None), "C0": dict(C=0), "C33": dict(C=33), "N0": dict(N=0),
                       "W0": dict(W=0), "too_many_pixels": dict(H=8193, W=8192), "out_misaligned": dict(out=OFF8),
                       "null_in+C0": dict(inp=None, C=0), "C33+N0": dict(C=33, N=0), "N0+out_misaligned": dict(N=0, out=OFF8)},
    "lnh_unet_conv3x3": dict(_CONV_FWD, **{"null_scale": dict(scale=None), "null_shift": dict(shift=None), "scale_misaligned": dict(scale=OFF8),
                                           "shift_misaligned": dict(shift=OFF8)}),
    "lnh_unet_conv3x3_raw": _CONV_FWD,
    "lnh_unet_upconv2x2": {"null_in": dict(inp=None), "null_weight": dict(weight=None), "null_bias": dict(bias=None), "null_out": dict(out=None),
                           "Cin_0": dict(Cin=0), "Cin_48": dict(Cin=48), "Cin_2048": dict(Cin=2048), "Cout_32": dict(Cout=32),
                           "Cout_96": dict(Cout=96), "Cout_2048": dict(Cout=2048), "N0": dict(N=0), "too_many_pixels": dict(H=4097, W=4096),
                           "in_misaligned": dict(inp=OFF8), "bias_misaligned": dict(bias=OFF8), "out_misaligned": dict(out=OFF8),
                           "null_in+Cin_48": dict(inp=None, Cin=48), "Cin_48+Cout_96": dict(Cin=48, Cout=96), "Cout_96+N0": dict(Cout=96, N=0),
                           "N0+in_misaligned": dict(N=0, inp=OFF8)},
    "lnh_unet_head": {"null_in": dict(inp=None), "null_weight": dict(weight=None), "null_bias": dict(bias=None), "null_logits": dict(logits=None),
                      "N0": dict(N=0), "too_many_pixels": dict(H=8193, W=8192), "in_misaligned": dict(inp=OFF8),
                      "weight_misaligned": dict(weight=OFF8), "null_in+N0": dict(inp=None, N=0), "N0+in_misaligned": dict(N=0, inp=OFF8)},
    "lnh_unet_pool_backward": {"null_x": dict(x=None), "null_dpool": dict(dpool=None), "null_dx": dict(dx=None), "C0": dict(C=0), "C48": dict(C=48),
                               "C2048": dict(C=2048), "N0": dict(N=0), "H0_1": dict(H0=1), "too_many_pixels": dict(H0=8193, W0=8192),
                               "stride_without_dskip": dict(skip_stride=128), "dskip_without_stride": dict(dskip=P),
                               "stride_below_C": dict(dskip=P, skip_stride=32), "stride_4": dict(dskip=P, skip_stride=68),
                               "stride_4096": dict(dskip=P, skip_stride=4096), "x_misaligned": dict(x=OFF8),
                               "dskip_misaligned": dict(dskip=OFF8, skip_stride=128), "null_x+C48": dict(x=None, C=48), "C48+N0": dict(C=48, N=0),
                               "N0+stride_without_dskip": dict(N=0, skip_stride=128), "stride_4+x_misaligned": dict(dskip=P, skip_stride=68, x=OFF8)},
    "lnh_unet_head_backward": {"null_a": dict(a=None), "null_weight": dict(weight=None), "null_dlogits": dict(dlogits=None), "null_ws": dict(ws=None),
                               "null_dx": dict(dx=None), "null_dweight": dict(dweight=None), "null_dbias": dict(dbias=None), "N0": dict(N=0),
                               "too_many_pixels": dict(H=8193, W=8192), "workspace_too_small": dict(ws_bytes=1039),
                               "a_misaligned": dict(a=OFF8), "ws_misaligned": dict(ws=OFF8), "dx_misaligned": dict(dx=OFF8),
                               "null_a+N0": dict(a=None, N=0), "N0+workspace_too_small": dict(N=0, ws_bytes=0),
                               "workspace_too_small+a_misaligned": dict(ws_bytes=1039, a=OFF8)},
    "lnh_unet_pack_upconv": {"null_weight": dict(weight=None), "null_fwd": dict(fwd=None), "Cin_32": dict(Cin=32), "Cin_96": dict(Cin=96),
                             "Cin_2048": dict(Cin=2048), "Cout_32": dict(Cout=32), "Cout_2048": dict(Cout=2048), "weight_misaligned": dict(weight=OFF8),
                             "bwd_misaligned": dict(bwd=OFF8), "null_weight+Cin_96": dict(weight=None, Cin=96), "Cin_96+Cout_32": dict(Cin=96, Cout=32),
                             "Cout_32+weight_misaligned": dict(Cout=32, weight=OFF8)},
    "lnh_unet_upconv2x2_backward_data": dict(_UP_BWD, **{"null_weight": dict(weight=None), "null_dx": dict(dx=None), "Cout_32_fits": dict(Cout=32, N=0),
                                                         "Cout_48": dict(Cout=48), "weight_misaligned": dict(weight=OFF8), "dx_misaligned": dict(dx=OFF8)}),
    "lnh_unet_upconv2x2_backward_weight": dict(_UP_BWD, **{"null_x": dict(x=None), "null_ws": dict(ws=None), "null_dweight": dict(dweight=None),
                                                           "null_dbias": dict(dbias=None), "Cout_32": dict(Cout=32), "Cout_96": dict(Cout=96),
                                                           "workspace_too_small": dict(ws_bytes=131327), "x_misaligned": dict(x=OFF8),
                                                           "ws_misaligned": dict(ws=OFF8), "offset_4+workspace_too_small": dict(dy_offset=4, ws_bytes=16),
                                                           "workspace_too_small+x_misaligned": dict(ws_bytes=16, x=OFF8)}),
    "lnh_unet_pack_conv3x3": {"null_weight": dict(weight=None), "null_fwd": dict(fwd=None), "Cout_0": dict(Cout=0), "Cout_96": dict(Cout=96),
                              "Cout_2048": dict(Cout=2048), "Cin_0": dict(Cin=0), "Cin_48": dict(Cin=48), "Cin_2048": dict(Cin=2048),
                              "bwd_with_Cin_10": dict(Cin=10), "bwd_with_Cin_96": dict(Cin=96), "weight_misaligned": dict(weight=OFF8),
                              "fwd_misaligned": dict(fwd=OFF8), "bwd_misaligned": dict(bwd=OFF8), "null_weight+Cout_96": dict(weight=None, Cout=96),
                              "Cout_96+Cin_48": dict(Cout=96, Cin=48), "Cin_48+weight_misaligned": dict(Cin=48, weight=OFF8),
                              "bwd_with_Cin_10+fwd_misaligned": dict(Cin=10, fwd=OFF8)},
    "lnh_unet_bn_stats": dict(_BN, **{"null_gamma": dict(gamma=None), "null_ws": dict(ws=None), "null_shift": dict(shift=None), "eps_negative": dict(eps=-1.0),
                                      "eps_nan": dict(eps=_NAN), "momentum_2": dict(momentum=2.0), "momentum_negative": dict(momentum=-0.5),
                                      "scale_misaligned": dict(scale=OFF8), "shift_misaligned": dict(shift=OFF8), "C48+eps_negative": dict(C=48, eps=-1.0),
                                      "eps_negative+workspace_too_small": dict(eps=-1.0, ws_bytes=16)}),
    "lnh_unet_bn_relu": {"null_z": dict(z=None), "null_scale": dict(scale=None), "null_a": dict(a=None), "M0": dict(M=0), "M_over": dict(M=(1 << 26) + 1),
                         "C0": dict(C=0), "C48": dict(C=48), "C2048": dict(C=2048), "z_misaligned": dict(z=OFF8), "scale_misaligned": dict(scale=OFF8),
                         "a_misaligned": dict(a=OFF8), "null_z+M0": dict(z=None, M=0), "M0+C48": dict(M=0, C=48), "C48+z_misaligned": dict(C=48, z=OFF8)},
    "lnh_unet_bn_relu_backward": dict(_BN, **{"null_a": dict(a=None), "null_da": dict(da=None), "null_mean": dict(mean=None), "null_ws": dict(ws=None),
                                              "null_dz": dict(dz=None), "null_dbeta": dict(dbeta=None), "a_misaligned": dict(a=OFF8),
                                              "da_misaligned": dict(da=OFF8), "dz_misaligned": dict(dz=OFF8)}),
    # (Cin = C0 + C1 beside a second source, so that the call reaches the checks behind that of Cin)
    "lnh_unet_conv3x3_backward_weight": dict({k: dict(v, Cin=128) if v.get("src1") and v.get("C1") == 64 else v for k, v in _CONV_SHARED.items()}, **{
        "null_dz": dict(dz=None), "null_ws": dict(ws=None), "null_dweight": dict(dweight=None), "C0_96": dict(C0=96, Cin=96),
        "C1_half_of_C0": dict(_CAT, C0=128, C1=64), "C1_beside_C0_32": dict(_CAT, C0=32, C1=32), "Cin_65": dict(Cin=65), "Cin_0_padded": dict(C0=32, Cin=0),
        "Cin_33_padded": dict(C0=32, Cin=33), "Cin_without_C1": dict(_CAT, Cin=64), "variant3": dict(variant=3), "workspace_too_small": dict(ws_bytes=147455),
        "dz_misaligned": dict(dz=OFF8), "ws_misaligned": dict(ws=OFF8), "dweight_misaligned": dict(dweight=OFF8), "Cout_96+Cin_65": dict(Cout=96, Cin=65),
        "Cin_65+N0": dict(Cin=65, N=0), "src1_taller+variant3": dict(_CAT, Cin=128, H1=17, variant=3), "variant3+workspace_too_small": dict(variant=3, ws_bytes=16),
        "workspace_too_small+dz_misaligned": dict(ws_bytes=16, dz=OFF8)}),
    "lnh_unet_loss_grad": {"null_logits": dict(logits=None), "null_masks": dict(masks=None), "null_ws": dict(ws=None), "null_loss": dict(loss=None),
                           "null_dlogits": dict(dlogits=None), "mask_dtype2": dict(mask_dtype=2), "M0": dict(M=0), "M_over": dict(M=(1 << 26) + 1),
                           "loss_scale_0": dict(loss_scale=0.0), "loss_scale_negative": dict(loss_scale=-1.0), "loss_scale_inf": dict(loss_scale=_INF),
                           "loss_scale_nan": dict(loss_scale=_NAN), "workspace_too_small": dict(ws_bytes=23), "logits_misaligned": dict(logits=P + 2),
                           "ws_misaligned": dict(ws=OFF4), "f32_masks_misaligned": dict(masks=P + 1), "null_logits+mask_dtype2": dict(logits=None, mask_dtype=2),
                           "mask_dtype2+M0": dict(mask_dtype=2, M=0), "M0+loss_scale_0": dict(M=0, loss_scale=0.0),
                           "loss_scale_0+workspace_too_small": dict(loss_scale=0.0, ws_bytes=23), "workspace_too_small+ws_misaligned": dict(ws_bytes=23, ws=OFF4)},
    "lnh_unet_grad_sumsq": dict(_TABLE, **{"null_ws": dict(ws=None), "ws_misaligned": dict(ws=OFF4), "workspace_too_small": dict(ws_bytes=8191),
                                           "n0+null_ws": dict(n=0, ws=None), "null_ws+workspace_too_small": dict(ws=None, ws_bytes=8191)}),
    "lnh_unet_rmsprop_step": dict(_TABLE, **{"loss_scale_0": dict(loss_scale=0.0), "loss_scale_inf": dict(loss_scale=_INF), "max_norm_0": dict(max_norm=0.0),
                                             "max_norm_nan": dict(max_norm=_NAN), "alpha_negative": dict(alpha=-0.1), "alpha_inf": dict(alpha=_INF),
                                             "eps_negative": dict(eps=-1e-8), "weight_decay_negative": dict(weight_decay=-1.0), "momentum_negative": dict(momentum=-0.5),
                                             "momentum_nan": dict(momentum=_NAN), "n0+loss_scale_0": dict(n=0, loss_scale=0.0),
                                             "loss_scale_0+max_norm_0": dict(loss_scale=0.0, max_norm=0.0), "max_norm_0+alpha_negative": dict(max_norm=0.0, alpha=-0.1),
                                             "alpha_negative+eps_negative": dict(alpha=-0.1, eps=-1e-8), "eps_negative+weight_decay_negative": dict(eps=-1e-8, weight_decay=-1.0),
                                             "weight_decay_negative+momentum_negative": dict(weight_decay=-1.0, momentum=-0.5)}),
}


def calls():
    """[(case name, entry point, argument list)]; the stream is appended by the caller."""
    return [(f"{fn}/{case}", fn, list(dict(BASES[fn], **delta).values())) for fn in BASES for case, delta in WRONG[fn].items()]


def _set_error_sentinel(lib):
    """A workspace-size function must leave lnh_last_error() alone: give it a known text to leave."""
    assert lib.lnh_sh_encode_forward(1, 1, 4, 3, 9, None, None) != 0
    return lib.lnh_last_error().decode()


def refusal_answers(lib, only=None):
    """{case: {"rc", "error"}}; `only`: the cases to call (the test passes those the record holds INVALID_ARG for)."""
    res = {}
    for name, fn, args in calls():
        if only is not None and name not in only:
            continue
        _set_error_sentinel(lib)
        rc = getattr(lib, fn)(*args, None)
        res[name] = {"rc": rc, "error": lib.lnh_last_error().decode()}
    return res


def _conv_layers(H, W):
    """(H0, W0, pool, C0, C1, Cout) of the 18 convolutions of the net on an H x W image, from the architecture alone."""
    sizes = [(H >> l, W >> l) for l in range(5)]
    out = [sizes[0] + (0, 32, 0, 64), sizes[0] + (0, 64, 0, 64)]
    for l in range(1, 5):
        out += [sizes[l - 1] + (1, CHANNELS[l - 1], 0, CHANNELS[l]), sizes[l] + (0, CHANNELS[l], 0, CHANNELS[l])]
    for l in (3, 2, 1, 0):
        out += [sizes[l] + (0, CHANNELS[l], CHANNELS[l], CHANNELS[l]), sizes[l] + (0, CHANNELS[l], 0, CHANNELS[l])]
    return out


def size_calls():
    """[(case name, size function, arguments)]: every *_workspace_size function on the levels of SHAPES and on what it answers 0 for."""
    out = [("lnh_unet_grad_sumsq_workspace_size", "lnh_unet_grad_sumsq_workspace_size", ())]
    for N, H, W in SHAPES:
        tag = f"{N}x{H}x{W}"
        out += [(f"lnh_unet_workspace_size/{tag}", "lnh_unet_workspace_size", (N, H, W)),
                (f"lnh_unet_head_backward_workspace_size/{tag}", "lnh_unet_head_backward_workspace_size", (N, H, W)),
                (f"lnh_unet_loss_grad_workspace_size/{tag}", "lnh_unet_loss_grad_workspace_size", (N * H * W,))]
        for l in range(4):
            a = (N, H >> (l + 1), W >> (l + 1), CHANNELS[l + 1], CHANNELS[l])
            out.append((f"lnh_unet_upconv2x2_backward_weight_workspace_size/{tag}/level{l}", "lnh_unet_upconv2x2_backward_weight_workspace_size", a))
        for k, (h0, w0, pool, c0, c1, cout) in enumerate(_conv_layers(H, W)):
            M = N * (h0 >> pool) * (w0 >> pool)
            out += [(f"lnh_unet_conv3x3_backward_weight_workspace_size/{tag}/layer{k}", "lnh_unet_conv3x3_backward_weight_workspace_size",
                     (N, h0, w0, pool, c0, c1, cout)),
                    (f"lnh_unet_bn_stats_workspace_size/{tag}/layer{k}", "lnh_unet_bn_stats_workspace_size", (M, cout)),
                    (f"lnh_unet_bn_relu_backward_workspace_size/{tag}/layer{k}", "lnh_unet_bn_relu_backward_workspace_size", (M, cout))]
    zero = {
        "lnh_unet_workspace_size": {"N0": (0, 16, 16), "H15": (1, 15, 16), "W15": (1, 16, 15), "too_many_pixels": (2, 8192, 8192)},
        "lnh_unet_head_backward_workspace_size": {"N0": (0, 16, 16), "W0": (1, 16, 0), "too_many_pixels": (1, 8193, 8192)},
        "lnh_unet_loss_grad_workspace_size": {"M0": (0,), "M_over": ((1 << 26) + 1,)},
        "lnh_unet_upconv2x2_backward_weight_workspace_size": {"N0": (0, 8, 8, 128, 64), "too_many_pixels": (1, 4097, 4096, 128, 64), "Cin_32": (1, 8, 8, 32, 64),
                                                              "Cin_96": (1, 8, 8, 96, 64), "Cout_32": (1, 8, 8, 128, 32), "Cout_2048": (1, 8, 8, 128, 2048)},
        "lnh_unet_conv3x3_backward_weight_workspace_size": {"N0": (0, 16, 16, 0, 64, 0, 64), "pool2": (1, 16, 16, 2, 64, 0, 64), "pooled_to_nothing": (1, 1, 16, 1, 64, 0, 64),
                                                            "too_many_pixels": (2, 8192, 8192, 0, 64, 0, 64), "C0_96": (1, 16, 16, 0, 96, 0, 64),
                                                            "C1_beside_C0_32": (1, 16, 16, 0, 32, 32, 64), "C1_half_of_C0": (1, 16, 16, 0, 128, 64, 64),
                                                            "Cout_96": (1, 16, 16, 0, 64, 0, 96)},
        "lnh_unet_bn_stats_workspace_size": {"M1": (1, 64), "M_over": ((1 << 26) + 1, 64), "C0": (256, 0), "C48": (256, 48), "C2048": (256, 2048)},
    }
    zero["lnh_unet_bn_relu_backward_workspace_size"] = zero["lnh_unet_bn_stats_workspace_size"]
    for fn, cases in zero.items():
        out += [(f"{fn}/zero/{case}", fn, a) for case, a in cases.items()]
    return out


def size_answers(lib):
    """{case: {"bytes", "error"}}: the answer, and the error text the function left (it must be the sentinel's)."""
    res = {}
    for name, fn, args in size_calls():
        _set_error_sentinel(lib)
        res[name] = {"bytes": int(getattr(lib, fn)(*args)), "error": lib.lnh_last_error().decode()}
    return res
