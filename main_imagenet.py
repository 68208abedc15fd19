"""Shifted-scale PTQ calibration driver (the README's entry point, README.md:20).

    python main_imagenet.py --device_gpu=cuda:0 --arch=resnet18 --n_bits_w=2 --n_bits_a=4 \
        --weight=1.0 --bias_cal=True --bias_ch_quant=True [--data_path DIR] [--checkpoint FP.pt]

Flow (the README flags mapped onto the snapshot's code):
  1. QuantModel(arch) with W n_bits_w per-channel / A n_bits_a per-tensor; 8-bit stem/head;
     weight delta/zp initialised on the first 64 calibration samples.
  2. --bias_ch_quant: every residual block is reconstructed with the fused shifted-scale
     loop (ChannelQuant 'adaShift', learns the input-channel shift group R); --bias_cal
     additionally learns gamma^z / phi^z.  Otherwise BRECQ AdaRound reconstruction.
     --opt_mode fisher_diag | fisher_full: BRECQ's loops use the Fisher-weighted loss.
  3. --act_quant: activation deltas initialised and reconstructed BRECQ-style (LSQ, p=2.4).
  4. Top-1 on --data_path/val.pt if present ("Weight quantization accuracy",
     "Full quantization (W{w}A{a}) accuracy"); otherwise the reconstruction losses.
Data: --data_path may hold cali.pt ([N,3,224,224] float) and val.pt ((images, labels));
without it synthetic N(0,1) calibration images are used (no network access here).
Multi-GPU: `--gpus N` spawns N rank processes (as the reference's mp.spawn,
Brecq/main_imagenet_dist.py:268-271), or launch with torch.distributed.run; each rank
calibrates on its shard of the calibration set and the per-iteration gradients are
all-reduced over RCCL.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

if __name__ == '__main__':
    # before torch is imported: the parent of the spawned ranks never loads the HIP runtime
    from shiftedscalequantization_amd.launch import maybe_spawn
    maybe_spawn(os.path.abspath(__file__))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from shiftedscalequantization_amd import drivers as D  # noqa: E402
from shiftedscalequantization_amd.cli import (parse_args, recon_kwargs, seed_all,  # noqa: E402
                                              validate_model)
from shiftedscalequantization_amd.parallel_dp import replicated, shard_rows  # noqa: E402
from shiftedscalequantization_amd.quant import QuantModule  # noqa: E402


def load_data(args, device):
    cali = val = None
    if args.data_path and os.path.exists(os.path.join(args.data_path, 'cali.pt')):
        cali = torch.load(os.path.join(args.data_path, 'cali.pt'), weights_only=True)
    if args.data_path and os.path.exists(os.path.join(args.data_path, 'val.pt')):
        val = torch.load(os.path.join(args.data_path, 'val.pt'), weights_only=True)
    if cali is None:
        g = torch.Generator().manual_seed(args.seed)
        cali = torch.randn(args.num_samples, 3, 224, 224, generator=g)
    lo, hi = shard_rows(len(cali))
    return cali[lo:hi].to(device), val


def val_loader(val, bs=256):
    """This rank's shard of the validation set in batches (validate_model all-reduces the
    per-rank sums)."""
    if val is None:
        return None
    images, labels = val
    lo, hi = shard_rows(len(images))
    images, labels = images[lo:hi], labels[lo:hi]
    return [(images[i:i + bs], labels[i:i + bs]) for i in range(0, len(images), bs)]


def run_integer_inference(qnn, args, cali, loader, bs=32):
    """Install the integer route the --int_infer* flags ask for, print the plan and validate
    (or run one batch) on it; --int_infer_graph: through a replayed HIP graph of the forward."""
    from shiftedscalequantization_amd.quant import (IntegerGraph, block_carry_report, carry_report,
                                                     enable_integer_inference,
                                                     head_carry_report, integer_report,
                                                     split_report, stem_carry_report)
    fused = {'fused_stem': True} if getattr(args, 'int_infer_fused_stem', False) else {}
    u8 = getattr(args, 'int_infer_u8_images', False)
    image_u8 = {'image_u8': (IMAGENET_MEAN, IMAGENET_STD)} if u8 else {}
    plan = enable_integer_inference(qnn, cali[:8], grouped=args.int_infer_grouped,
                                    carry=args.int_infer_carry,
                                    carry_blocks=args.int_infer_carry_blocks,
                                    carry_stem=args.int_infer_carry_stem,
                                    carry_head=args.int_infer_carry_head,
                                    colscale=args.int_infer_colscale,
                                    splitk=args.int_infer_splitk,
                                    per_ci=args.int_infer_per_ci, wide=args.int_infer_wide,
                                    wide_all=getattr(args, 'int_infer_wide_all', False),
                                    **fused, **image_u8)
    n_int = sum(v == 'int8' for v in plan.values())
    print(f'integer inference: {n_int} of {len(plan)} layers on int8 codes')
    if args.int_infer_carry:
        pairs = carry_report(qnn)['pairs']
        print(f'integer inference: int8 codes carried between {len(pairs)} pairs: '
              + ', '.join(f'{a} -> {b}' for a, b in pairs))
    if args.int_infer_carry_blocks:
        edges = block_carry_report(qnn)['edges']
        print(f'integer inference: int8 codes carried across {len(edges)} block edges: '
              + ', '.join(f'{a} -> {b}' for a, b in edges))
    if args.int_infer_carry_stem:
        edges = stem_carry_report(qnn)['edges']
        print(f'integer inference: int8 codes carried from {len(edges)} stem edges: '
              + ', '.join(' -> '.join([a] + pools + [b]) for a, pools, b in edges))
    if fused:
        why = stem_carry_report(qnn)['unfused']
        print('integer inference: stem conv emitting its own codes (K31): '
              + ', '.join(f'{n}: {"yes" if not w else w}' for n, w in why.items()))
    if u8:
        print('integer inference: uint8 images, stem conv on the int8 MFMA (K32): '
              + ', '.join(f'{n}: {"yes" if not w else w}' for n, w in qnn._int_u8.items()))
    if args.int_infer_carry_head:
        edges = head_carry_report(qnn)['edges']
        print(f'integer inference: int8 codes carried to the logits along {len(edges)} head '
              'edges: ' + ', '.join(' -> '.join(e) for e in edges))
    for name, why in plan.items():
        print(f'  {name}: {why}')
    if u8:
        run_u8_images(qnn, args, cali, loader, bs)
    elif loader is not None:
        acc = validate_model(loader, qnn, graph=args.int_infer_graph)
        print('Integer inference (W{}A{}) accuracy: {}'.format(args.n_bits_w, args.n_bits_a, acc))
    elif args.int_infer_graph:
        IntegerGraph(qnn)(cali[:bs])
    else:
        with torch.no_grad():
            qnn(cali[:bs])
    if args.int_infer_splitk:
        split = {n: z for n, z in split_report(qnn).items() if z > 1}
        print(f'integer inference: {len(split)} layers split along K: '
              + ', '.join(f'{n} x{z}' for n, z in split.items()))
    print(f'integer inference: {integer_report(qnn)["off_grid"]} off-grid activations')


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def to_u8(images):
    """A float image batch back on the loader's uint8 grid; a uint8 batch passes as it is.  A float
    batch is taken to be normalised with IMAGENET_MEAN / IMAGENET_STD, the values `image_u8` gets:
    a validation set normalised otherwise has to be stored as uint8."""
    if images.dtype == torch.uint8:
        return images
    mean = torch.tensor(IMAGENET_MEAN, device=images.device).reshape(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=images.device).reshape(1, 3, 1, 1)
    return ((images * std + mean) * 255).round().clamp(0, 255).to(torch.uint8)


def u8_view(u, layout='nchw'):
    """The uint8 batch `u` (N, 3, H, W) laid out as --int_infer_u8_layout says and handed back as an
    (N, 3, H, W) view of it: 'nhwc' interleaved pixels, 'rgba' 4-byte pixels whose last byte is a
    pad (255); 'nchw' is `u` itself."""
    if layout == 'nchw':
        return u
    px = u.permute(0, 2, 3, 1)
    if layout == 'rgba':
        px = torch.cat([px, torch.full_like(px[..., :1], 255)], dim=3)
    return px.contiguous()[..., :3].permute(0, 3, 1, 2)


def run_u8_images(qnn, args, cali, loader, bs):
    """--int_infer_u8_images: validation (or one synthetic batch drawn as uint8) on uint8 images,
    then the same batches normalised to fp32 through the same plan, and the stem report."""
    from shiftedscalequantization_amd.quant import IntegerGraph, integer_report, stem_carry_report
    from shiftedscalequantization_amd.quant.integer import normalise_u8
    layout = getattr(args, 'int_infer_u8_layout', 'nchw')
    frame = getattr(args, 'int_infer_u8_frame', 0)
    dev = cali.device
    mean = torch.tensor(IMAGENET_MEAN, device=dev).reshape(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=dev).reshape(1, 3, 1, 1)
    if loader is not None:
        # one batch at a time in each pass: no second copy of the validation set
        acc = validate_model(((u8_view(to_u8(x), layout), t) for x, t in loader), qnn,
                             graph=args.int_infer_graph)
        print('Integer inference on uint8 images (W{}A{}) accuracy: {}'.format(
            args.n_bits_w, args.n_bits_a, acc))
        acc = validate_model(((normalise_u8(to_u8(x), mean.cpu(), std.cpu()), t) for x, t in loader),
                             qnn, graph=args.int_infer_graph)
        print('Integer inference on the same images normalised to fp32 (W{}A{}) accuracy: {}'.format(
            args.n_bits_w, args.n_bits_a, acc))
    else:
        g = torch.Generator().manual_seed(args.seed)
        C, H, W = (int(v) for v in cali.shape[1:])
        if frame and (frame < H or frame < W):
            raise SystemExit(f'--int_infer_u8_frame {frame} is smaller than the input {H} x {W}')
        FH, FW = (frame, frame) if frame else (H, W)
        u = torch.randint(0, 256, (bs, C, FH, FW), generator=g, dtype=torch.uint8).to(dev)
        top, left = (FH - H) // 2, (FW - W) // 2
        u = u8_view(u, layout)[:, :, top:top + H, left:left + W]      # the centre crop, a view
        forward = IntegerGraph(qnn) if args.int_infer_graph else qnn
        with torch.no_grad():
            out_u8 = forward(u).clone()
            out_f32 = forward(normalise_u8(u.contiguous(), mean, std)).clone()
        diff = (out_u8 - out_f32).abs().max().item()
        same = (out_u8.argmax(1) == out_f32.argmax(1)).float().mean().item()
        print(f'integer inference: one uint8 batch of {bs}: max |logit difference| to the same batch '
              f'normalised to fp32 {diff:.4g}, same top-1 on {100 * same:.1f}%')
    rep = stem_carry_report(qnn)
    print(f'integer inference: uint8 stem forwards on K32: {rep["u8"]}; normalised on the device '
          f'instead, by reason: {rep["un_u8"]}')
    print(f'integer inference: uint8 stem forwards on K32 by staging form ({layout}'
          + (f', {frame} x {frame} frames cropped' if frame else '')
          + f'): {integer_report(qnn)["u8_form"]}')


def main(argv=None):
    args = parse_args(argv)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world > 1:
        # one process per GPU; ranks beyond the visible GPUs share them (gloo rehearsals)
        local = int(os.environ.get('LOCAL_RANK', '0'))
        ndev = torch.cuda.device_count()
        if args.dist_backend == 'nccl' and world > ndev:
            raise SystemExit(f'main_imagenet.py: {world} ranks over RCCL need {world} GPUs, {ndev} '
                             f'visible (rehearse with --dist_backend gloo: ranks then share devices)')
        device = torch.device('cuda', local % max(ndev, 1))
        torch.cuda.set_device(device)
        if args.dist_backend == 'nccl':
            dist.init_process_group('nccl', device_id=device)
        else:
            dist.init_process_group(args.dist_backend)
    else:
        device = torch.device(args.device_gpu)
    seed_all(args.seed, deterministic=bool(args.deterministic))
    cali, val = load_data(args, device)
    loader = val_loader(val)
    t0 = time.time()
    qnn = D.build_qnn(args.arch, args.n_bits_w, args.n_bits_a, args.channel_wise, args.w_scale_method,
                      args.a_scale_method, device, args.checkpoint, args.disable_8bit_head_stem)
    if args.test:
        # the shipped default (`ShiftedScaleQuant.py --test=True` -> channelShift_wMSE,
        # :119-183): input-channel scales by the ChannelQuantMSE range test, no recon loop
        shifts = [float(s) for s in args.shift_targets.split(',')]
        fc = [n for n, m in qnn.named_modules() if isinstance(m, QuantModule)][-1]
        D.channelShift_wMSE(qnn, cali, level=args.mse_level, threshold=args.mse_threshold,
                            opt_mode=args.shift_quant_mode, shiftTarget=shifts,
                            layerDisabled=['.' + fc])
        torch.cuda.synchronize(device)
        acc = validate_model(loader, qnn) if loader is not None else None
        print(f'channelShift_wMSE (level {args.mse_level}, threshold {args.mse_threshold}) '
              f'finished in {time.time() - t0:.1f}s; accuracy of qnn_hard: {acc}')
        if args.int_infer_colscale:
            # the shipped path on integer codes: the column-scaled weights on their common
            # integer grid, the act quantizers initialised on the calibration head
            qnn.set_quant_state(True, True)
            with torch.no_grad():
                qnn(cali[:64])
            if world > 1:
                qnn.synchorize_activation_statistics()
            qnn.disable_network_output_quantization()
            run_integer_inference(qnn, args, cali, loader)
        if world > 1:
            dist.destroy_process_group()
        return qnn
    qnn.set_quant_state(True, False)
    with torch.no_grad():
        qnn(cali[:64])
    bs = 32
    report = {}
    phases = {'init': time.time() - t0}
    t_phase = time.time()
    if args.bias_ch_quant:
        shifts = [float(s) for s in args.shift_targets.split(',')]
        blocks = D.block_paths(qnn)
        D.build_ShiftedChannelQuant(qnn, blocks, '', shiftTarget=shifts, skipShiftLayer=[])
        qnn.set_quant_state(False, False)
        for path in blocks:
            D.cache_block_features(qnn, path, cali, bs, device)
            D.set_quant_state_block(qnn, [path], '', True)
            res = D.QuantRecursiveShiftRecon(qnn, [path], qnn, loader, iters=args.shift_iters,
                                             lmda=0.1 * args.weight, lmdaR=0.01 * args.weight,
                                             bias_cal=args.bias_cal)
            report.update(res)
            D.find_module(qnn, path).clear_cached_features()
        # the remaining single layers (fc) with BRECQ AdaRound
        last = [m for m in qnn.modules() if isinstance(m, QuantModule)][-1]
        from shiftedscalequantization_amd.quant import layer_reconstruction
        layer_reconstruction(qnn, last, cali, **dict(recon_kwargs(args, False, bs), weight=0.01))
    else:
        D.recon_model(qnn, qnn, cali_data=cali, **recon_kwargs(args, False, bs))
    torch.cuda.synchronize(device)
    phases['weight_recon'] = time.time() - t_phase
    t_phase = time.time()
    qnn.set_quant_state(weight_quant=True, act_quant=False)
    if loader is not None:
        print('Weight quantization accuracy: {}'.format(validate_model(loader, qnn)))
    if args.act_quant:
        qnn.set_quant_state(True, True)
        with torch.no_grad():
            qnn(cali[:64])
        if world > 1:
            # each rank initialised its act deltas on its own shard: all-average them
            # (Brecq/main_imagenet_dist.py:210-211) so the act phase starts replicated
            qnn.synchorize_activation_statistics()
        qnn.disable_network_output_quantization()
        D.recon_model(qnn, qnn, cali_data=cali, **recon_kwargs(args, True, bs))
        qnn.set_quant_state(weight_quant=True, act_quant=True)
        torch.cuda.synchronize(device)
        phases['act_recon'] = time.time() - t_phase
        if loader is not None:
            print('Full quantization (W{}A{}) accuracy: {}'.format(args.n_bits_w, args.n_bits_a,
                                                                   validate_model(loader, qnn)))
        if args.act_shift:
            # the activation half of the shifted scale: per block, which of delta * s_i each
            # activation channel uses (K33); top-1 after it is not pinned by any golden
            t_phase = time.time()
            shifts = [float(s) for s in args.act_shift_targets.split(',')]
            act_report = D.act_shift_recon(qnn, cali, bs, device, shifts, args.act_shift_iters)
            qnn.set_quant_state(weight_quant=True, act_quant=True)
            torch.cuda.synchronize(device)
            phases['act_shift'] = time.time() - t_phase
            print(f'activation shift rec losses [soft, hard] per block: {act_report}')
            if loader is not None:
                print('Shifted activations (W{}A{}) accuracy: {}'.format(
                    args.n_bits_w, args.n_bits_a, validate_model(loader, qnn)))
    if args.int_infer and args.act_quant:
        run_integer_inference(qnn, args, cali, loader, bs)
    print(f'calibration finished in {time.time() - t0:.1f}s '
          f'({", ".join(f"{k} {v:.1f}s" for k, v in phases.items())}); block rec losses: '
          f'{ {k: v for k, v in report.items()} }')
    if world > 1:
        # the calibrated model (learned shift logits, AdaRound V, gamma^z/phi^z, act deltas)
        # must be bit-identical on every rank
        print(f'rank {dist.get_rank()}/{world}: calibrated model replicated across ranks: '
              f'{replicated(qnn)}')
        dist.destroy_process_group()
    return qnn


if __name__ == '__main__':
    main()
