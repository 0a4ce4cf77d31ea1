"""Functional torch restatement of the residual V-Net family (has_residual=True; a helper module, not a conftest).

ResidualConvBlock (code/networks/vnet.py:37-67): stages 0 .. n-2 are Conv3d 3^3 -> BatchNorm3d -> ReLU, the last stage Conv3d ->
BatchNorm3d without ReLU, then out = ReLU(last + x) with x the block's input; the encoder and the decoders are those of
oracle.nets.vnet_encoder / vnet_decoder with that block (vnet.py:127-223).  State dicts are the reference's checkpoints (the keys of
has_residual=False); dropout keep masks are injected as in oracle.nets.  Any floating dtype: the state dict's.  Pinned against the
imported reference by tests/golden/vnet_residual_32.npz (tools/gen_golden_residual.py)."""
import torch.nn.functional as F

from oracle.nets import VNET_DEC, VNET_STAGES, Ctx, _bn, _drop


def residual_block(sd, pre, x, n_stages, ctx):
    y = x
    for s in range(n_stages):
        y = F.conv3d(y, sd["%s.conv.%d.weight" % (pre, 3 * s)], sd["%s.conv.%d.bias" % (pre, 3 * s)], padding=1)
        y = _bn(sd, "%s.conv.%d" % (pre, 3 * s + 1), y, ctx)
        if s != n_stages - 1:
            y = F.relu(y)
    return F.relu(y + x)            # block_one: x [N, 1, ...] broadcasts over the 16 channels


def encoder(sd, x, ctx, has_dropout):
    feats = []
    for i, (name, n) in enumerate(VNET_STAGES):
        x = residual_block(sd, "encoder.block_" + name, x, n, ctx)
        if i < 4:
            feats.append(x)
            dw = "encoder.block_%s_dw" % name
            x = F.relu(_bn(sd, dw + ".conv.1", F.conv3d(x, sd[dw + ".conv.0.weight"], sd[dw + ".conv.0.bias"], stride=2), ctx))
    if has_dropout:
        x = _drop(x, "encoder.dropout", 0.5, ctx)
    feats.append(x)
    return feats


def decoder(sd, root, feats, ctx, has_dropout):
    trilinear = sd[root + ".block_five_up.conv.1.weight"].dim() == 5
    x = feats[4]
    for k, (upn, blk, n) in enumerate(VNET_DEC):
        up = "%s.block_%s" % (root, upn)
        if trilinear:
            x = F.interpolate(x, scale_factor=2, mode="trilinear", align_corners=True)
            x = F.relu(_bn(sd, up + ".conv.2", F.conv3d(x, sd[up + ".conv.1.weight"], sd[up + ".conv.1.bias"], padding=1), ctx))
        else:
            x = F.relu(_bn(sd, up + ".conv.1", F.conv_transpose3d(x, sd[up + ".conv.0.weight"], sd[up + ".conv.0.bias"], stride=2), ctx))
        x = residual_block(sd, "%s.block_%s" % (root, blk), x + feats[3 - k], n, ctx)
    if has_dropout:
        x = _drop(x, root + ".dropout", 0.5, ctx)
    return F.conv3d(x, sd[root + ".out_conv.weight"], sd[root + ".out_conv.bias"])


def dual_decoder_3d(sd, x, train=False, drop=None, update_stats=True, has_dropout=True):
    ctx = Ctx(train, drop, update_stats)
    feats = encoder(sd, x, ctx, has_dropout)
    return decoder(sd, "decoder1", feats, ctx, has_dropout), decoder(sd, "decoder2", feats, ctx, has_dropout)


def vnet_3d(sd, x, train=False, drop=None, update_stats=True, has_dropout=True):
    ctx = Ctx(train, drop, update_stats)
    return decoder(sd, "decoder", encoder(sd, x, ctx, has_dropout), ctx, has_dropout)


def cast_state(sd, dtype):
    """A copy of a state dict with the floating tensors in `dtype` (the integer num_batches_tracked kept)."""
    return {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
