"""Command-line flags of the calibration driver (main_imagenet.py).

Union of the README's command (README.md:20: --device_gpu --arch --n_bits_w --n_bits_a
--weight --bias_cal --bias_ch_quant), the shifted-scale driver's flags (common.py:19-75)
and BRECQ's (Brecq/main_imagenet.py:135-169).  Boolean flags keep the reference's
`type=bool` parsing (any non-empty string, "False" included, is True) so existing
command lines behave identically.
"""
import argparse
import os
import random

import numpy as np
import torch


def build_parser():
    p = argparse.ArgumentParser(description='running parameters',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    # general
    p.add_argument('--seed', default=1005, type=int)
    p.add_argument('--arch', default='resnet18', type=str,
                   choices=['resnet18', 'resnet34', 'resnet50', 'mobilenetv2', 'regnetx_600m',
                            'regnetx_3200m', 'mnasnet'])
    p.add_argument('--batch_size', default=64, type=int)
    p.add_argument('--workers', default=4, type=int)
    p.add_argument('--data_path', default='', type=str,
                   help='directory with cali.pt / val.pt tensors; empty -> synthetic data')
    p.add_argument('--checkpoint', default='', type=str, help='FP state_dict (weights_only load)')
    p.add_argument('--device_gpu', default='cuda:0', type=str)
    p.add_argument('--run_device', default='', type=str, help='alias of --device_gpu (common.py)')
    # quantization
    p.add_argument('--n_bits_w', default=2, type=int)
    p.add_argument('--channel_wise', default=True, type=bool)
    p.add_argument('--n_bits_a', default=4, type=int)
    p.add_argument('--act_quant', default=True, type=bool)
    p.add_argument('--disable_8bit_head_stem', default=False, type=bool)
    p.add_argument('--test_before_calibration', default=False, type=bool)
    p.add_argument('--w_scale_method', default='mse', type=str)
    p.add_argument('--a_scale_method', default='mse', type=str)
    # weight calibration
    p.add_argument('--num_samples', default=1024, type=int)
    p.add_argument('--iters_w', default=20000, type=int)
    p.add_argument('--weight', default=0.01, type=float,
                   help='lambda of the rounding and group (shift) policy')
    p.add_argument('--sym', default=False, type=bool)
    p.add_argument('--b_start', default=20, type=int)
    p.add_argument('--b_end', default=2, type=int)
    p.add_argument('--warmup', default=0.2, type=float)
    p.add_argument('--step', default=20, type=int)
    p.add_argument('--opt_mode', default='mse', type=str,
                   choices=['mse', 'fisher_diag', 'fisher_full'],
                   help="BRECQ's reconstruction loss: squared error, or weighted by the cached "
                        "|dKL/d(output)| + 1 (Fisher diagonal / per-sample full approximation)")
    # activation calibration
    p.add_argument('--iters_a', default=5000, type=int)
    p.add_argument('--lr', default=4e-4, type=float)
    p.add_argument('--p', default=2.4, type=float)
    # shifted-scale (README "Key Options")
    p.add_argument('--bias_cal', default=False, type=bool,
                   help='learn the output-channel scale gamma^z and offset phi^z')
    p.add_argument('--bias_ch_quant', default=False, type=bool,
                   help='learn the input-channel shift group R (fused shifted-scale recon)')
    p.add_argument('--shift_iters', default=625, type=int,
                   help='iterations of the fused shifted-scale recon (ShiftedScaleQuant.py:386)')
    p.add_argument('--shift_targets', default='0.96875,1.03125,1.0', type=str)
    p.add_argument('--mse_level', default=1, type=int)
    p.add_argument('--mse_threshold', default=1.0, type=float)
    p.add_argument('--shift_quant_mode', default='max', type=str)
    p.add_argument('--test', default=False, type=bool, help='ChannelQuantMSE path (channelShift_wMSE)')
    p.add_argument('--skip_test', default=False, type=bool)
    p.add_argument('--keep_features_on_host', default=False, type=bool)
    p.add_argument('--act_shift', action='store_true',
                   help='after the act phase, learn per block which shifted scale delta * s_i each '
                        'activation channel uses (ChannelQuantAct, K33); needs --act_quant')
    p.add_argument('--act_shift_targets', default='1.0,0.5', type=str,
                   help='the scale multipliers s_i of --act_shift (at most 4)')
    p.add_argument('--act_shift_iters', default=625, type=int,
                   help='iterations of the --act_shift loop per block')
    p.add_argument('--int_infer', action='store_true',
                   help='after calibration, validate again with the interior layers on their '
                        'integer codes (int8 MFMA conv / linear) and print the per-layer report')
    p.add_argument('--int_infer_grouped', action='store_true',
                   help='--int_infer with the grouped and depthwise convs on integer codes too '
                        '(depthwise direct kernel, grouped int8 MFMA conv); implies --int_infer')
    p.add_argument('--int_infer_carry', action='store_true',
                   help='--int_infer with int8 codes carried between the integer layers of a '
                        'block (conv, epilogue and act quantizer in one kernel, no fp32 tensor '
                        'in between); implies --int_infer')
    p.add_argument('--int_infer_carry_blocks', action='store_true',
                   help='--int_infer_carry with the codes also carried across block tails '
                        '(residual add in the conv kernel) and block boundaries; implies '
                        '--int_infer_carry and --int_infer')
    p.add_argument('--int_infer_carry_stem', action='store_true',
                   help='--int_infer_carry_blocks with the codes starting at the stem: its '
                        'epilogue emits int8 codes and a max-pool behind it pools them; implies '
                        '--int_infer_carry_blocks')
    p.add_argument('--int_infer_carry_head', action='store_true',
                   help='--int_infer_carry_stem with the codes running to the logits: the global '
                        'average pool sums the int8 codes and the fc runs on the sums (a numerics '
                        'contract of its own, DESIGN 4); implies --int_infer_carry_stem')
    p.add_argument('--int_infer_fused_stem', action='store_true',
                   help='--int_infer_carry_stem with the stem conv itself emitting the int8 codes '
                        '(fp32-MFMA conv with a stated summation order, no fp32 tensor and no '
                        'library conv; DESIGN 4 "Fused stem (K31)"); implies --int_infer_carry_stem')
    p.add_argument('--int_infer_u8_images', action='store_true',
                   help='with --int_infer_carry_stem or --int_infer_carry_head: the integer route is '
                        'fed uint8 images (x = (u/255 - mean)/std, the ImageNet mean / std) and the '
                        'stem conv runs on the int8 MFMA (K32; DESIGN 4 "uint8 stem (K32)"); it '
                        'implies none of them and is an error without a stem edge')
    p.add_argument('--int_infer_u8_layout', choices=('nchw', 'nhwc', 'rgba'), default='nchw',
                   help='with --int_infer_u8_images: how the uint8 batch lies in memory -- planar '
                        '(N, 3, H, W), interleaved (N, H, W, 3), or (N, H, W, 4) with a pad byte; '
                        'the interleaved ones are handed over as views, read in place where the '
                        'shape rule lets them (DESIGN 4 "uint8 stem (K32)", Strided views; '
                        'SSQ_STEM_U8_STRIDED=auto|1|0)')
    p.add_argument('--int_infer_u8_frame', type=int, default=0, metavar='F',
                   help='with --int_infer_u8_images and no --data_path: the synthetic uint8 batch '
                        'is drawn as F x F frames and centre-cropped to the input size as a view')
    p.add_argument('--int_infer_colscale', action='store_true',
                   help='--int_infer with column-scaled weights (ChannelQuantMSE, the --test path) '
                        'on integer codes too: the column scale as integers k / L, L <= 127, folded '
                        'into the int8 weight operand; with --test the act quantizers are '
                        'initialised and the route runs after channelShift_wMSE; implies --int_infer')
    p.add_argument('--int_infer_per_ci', action='store_true',
                   help='--int_infer with weights scaled per (co, ci) (ChannelQuant shifted scales: '
                        'the layer / block shiftedScale reconstructions) on integer codes too: the '
                        'scale as base[co] * k / L, the integer k folded into the int8 weight '
                        'operand; implies --int_infer')
    p.add_argument('--int_infer_wide', action='store_true',
                   help='--int_infer with a scaled weight operand (q - z) * k that leaves int8 run '
                        'as two int8 digits (|m| <= 16319, L <= 1024) instead of being refused; '
                        'goes with --int_infer_per_ci / --int_infer_colscale; implies --int_infer')
    p.add_argument('--int_infer_wide_all', action='store_true',
                   help='--int_infer_wide with the two-digit operand also on grouped and depthwise '
                        'convs and on the pooled-operand fc of --int_infer_carry_head (which then '
                        'takes a scaled fc); implies --int_infer_wide')
    p.add_argument('--int_infer_splitk', action='store_true',
                   help='--int_infer with the dense int8 convs of small planes split along K '
                        'where the host rule asks for it (two kernels, bit-identical); implies '
                        '--int_infer')
    p.add_argument('--int_infer_graph', action='store_true',
                   help='--int_infer with the integer forward captured once per batch shape and '
                        'replayed as one HIP graph; implies --int_infer')
    p.add_argument('--deterministic', default=1, type=int,
                   help='1 (reference): deterministic MIOpen conv solvers; 0: fastest solvers')
    # data parallel: one process per GPU, spawned by main_imagenet.py itself with --gpus N
    # (the reference's mp.spawn, Brecq/main_imagenet_dist.py:268-271) or by an external
    # torch.distributed.run
    p.add_argument('--gpus', default=1, type=int,
                   help='ranks to spawn on this node (one per GPU) when no launcher set WORLD_SIZE')
    p.add_argument('--dist_backend', default='nccl', type=str,
                   help="torch.distributed backend for world > 1: 'nccl' (= RCCL over xGMI); "
                        "'gloo' rehearses several ranks on one GPU")
    return p


def parse_args(argv=None):
    parser = build_parser()
    a = parser.parse_args(argv)
    if a.run_device:
        a.device_gpu = a.run_device
    if a.act_shift:
        if not a.act_quant:
            parser.error('--act_shift learns the activation quantizers: it needs --act_quant')
        if not 1 <= len(a.act_shift_targets.split(',')) <= 4:
            parser.error('--act_shift_targets takes 1 to 4 scale multipliers')
        if int(os.environ.get('WORLD_SIZE', '1')) > 1 or a.gpus > 1:
            parser.error('--act_shift runs on one device (world 1)')
    if a.int_infer_carry_head or a.int_infer_fused_stem:
        a.int_infer_carry_stem = True
    if a.int_infer_u8_images and not a.int_infer_carry_stem:
        parser.error('--int_infer_u8_images needs a stem edge: --int_infer_carry_stem, '
                     '--int_infer_carry_head or --int_infer_fused_stem')
    if (a.int_infer_u8_layout != 'nchw' or a.int_infer_u8_frame) and not a.int_infer_u8_images:
        parser.error('--int_infer_u8_layout / --int_infer_u8_frame need --int_infer_u8_images')
    if a.int_infer_u8_frame < 0:
        parser.error('--int_infer_u8_frame must be positive')
    if a.int_infer_carry_stem:
        a.int_infer_carry_blocks = True
    if a.int_infer_carry_blocks:
        a.int_infer_carry = True
    if a.int_infer_wide_all:
        a.int_infer_wide = True
    if (a.int_infer_grouped or a.int_infer_carry or a.int_infer_colscale or a.int_infer_splitk
            or a.int_infer_graph or a.int_infer_per_ci or a.int_infer_wide):
        a.int_infer = True
    return a


def recon_kwargs(args, act_quant, batch_size=32):
    """The keyword arguments main_imagenet.py hands to BRECQ's block / layer reconstruction
    (Brecq/main_imagenet.py:196-241): the AdaRound weight phase, or the act-delta phase."""
    if act_quant:
        return dict(iters=args.iters_a, act_quant=True, opt_mode=args.opt_mode, lr=args.lr,
                    p=args.p, batch_size=batch_size)
    return dict(iters=args.iters_w, weight=args.weight, asym=True,
                b_range=(args.b_start, args.b_end), warmup=args.warmup, act_quant=False,
                opt_mode=args.opt_mode, batch_size=batch_size)


def seed_all(seed=1029, deterministic=True):
    """common.py:77-85.  deterministic=True (the reference's setting) restricts MIOpen to
    deterministic convolution solvers -- for some stride-2 / 1x1 weight gradients that is a
    naive kernel; False lets MIOpen pick its fastest solvers (the ssq kernels are
    deterministic either way)."""
    random.seed(seed)
    os.environ['PYTHONHASHSEED'] = str(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    torch.backends.cudnn.benchmark = False
    torch.backends.cudnn.deterministic = bool(deterministic)


def accuracy(output, target, topk=(1,)):
    """common.py:128-142."""
    with torch.no_grad():
        maxk = max(topk)
        bs = target.size(0)
        _, pred = output.topk(maxk, 1, True, True)
        correct = pred.t().eq(target.view(1, -1).expand_as(pred.t()))
        return [correct[:k].reshape(-1).float().sum(0, keepdim=True).mul_(100.0 / bs) for k in topk]


def get_train_samples(train_loader, num_samples):
    """common.py:144-150."""
    data = []
    for batch in train_loader:
        data.append(batch[0])
        if len(data) * batch[0].size(0) >= num_samples:
            break
    return torch.cat(data, dim=0)[:num_samples]


@torch.no_grad()
def validate_model(val_loader, model, device=None, print_result=False, graph=False):
    """common.py:152-221: top-1 over (images, target) batches.  With several ranks each
    validates its own shard of the validation set and the (correct, total) sums are
    all-reduced (Brecq/main_imagenet_dist.py:114-124), so every rank returns the
    whole-set top-1.  `graph`: every batch goes through a quant.IntegerGraph of `model`
    (an installed integer plan, one capture per batch shape); each batch's static logits are
    reduced before the next replay, the all-reduce stays outside."""
    from .parallel_dp import all_sum_
    from .quant.quant_layer import frozen_weight_cache
    device = next(model.parameters()).device if device is None else device
    model.eval()
    forward = model
    if graph:
        from .quant.integer import IntegerGraph
        forward = IntegerGraph(model)
    sums = torch.zeros(2, dtype=torch.float64, device=device)
    # every layer's W_hat is quantized once per pass, not once per batch (bit-identical)
    with frozen_weight_cache():
        for images, target in val_loader:
            out = forward(images.to(device))
            sums[0] += (out.argmax(1) == target.to(device)).sum()
            sums[1] += target.numel()
    all_sum_(sums)
    correct, total = sums.tolist()
    acc = 100.0 * correct / max(total, 1)
    if print_result:
        print(f' * Acc@1 {acc:.3f}')
    return acc
