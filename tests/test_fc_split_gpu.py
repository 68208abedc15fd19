"""K19 split around the gradient all-reduce (ssq_fc_recon_grad + ssq_fc_recon_apply,
block_recon.FC_SPLIT): the pair against the fused ssq_fc_recon_iter, bit for bit -- one
iteration at the kernel level, a foreign (summed, bucket-sliced) gradient through the apply
half, and BRECQ's layer loop at world 1 with the split forced on."""
import importlib

import numpy as np
import pytest
import torch

import test_recon_gpu as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from shiftedscalequantization_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def Q(K):
    from shiftedscalequantization_amd import quant
    return quant


def bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.int32)


def same_bits(a, b, what=""):
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=what)


def fc_inputs(K, bs, Co, Ci, lam, step=7):
    """test_fc_recon_iter_vs_reference's inputs: seeded caches, weight, 8-bit per-row scale,
    V off its initial value, non-zero Adam moments, the slot of iteration `step`."""
    gen = torch.Generator().manual_seed(bs + Co)
    N = 3 * bs
    x = torch.relu(torch.randn(N, Ci, generator=gen)).cuda()
    tgt = torch.randn(N, Co, generator=gen).cuda()
    w = (0.05 * torch.randn(Co, Ci, generator=gen)).cuda()
    bias = (0.1 * torch.randn(Co, generator=gen)).cuda()
    d, z, _ = K.scale_init(w, 8, False, True, "max")
    v = K.rect_init(w, d)
    v += (0.3 * torch.randn(Co, Ci, generator=gen)).cuda()
    m = (1e-3 * torch.randn(Co, Ci, generator=gen)).cuda()
    s2 = (1e-6 * torch.rand(Co, Ci, generator=gen)).cuda()
    idx = [torch.randperm(N, generator=gen)[:bs] for _ in range(2)]

    def slot(k):
        sl = torch.zeros(bs + 2, dtype=torch.int64)
        sl[:bs] = idx[k]
        t = step + k
        words = np.array([lam, 12.5, -1e-3 / (1 - 0.9 ** t), (1 - 0.999 ** t) ** 0.5], np.float32)
        sl[bs:] = torch.from_numpy(words.view(np.int64))
        return sl.cuda(), words

    what = K.adaround(v, w, d, z, 8, False, False).detach().clone()
    return dict(x=x, tgt=tgt, w=w, bias=bias, d=d, z=z, v=v, m=m, s2=s2, what=what,
                slots=[slot(0), slot(1)])


@pytest.mark.parametrize("bs,Co,Ci,lam", [(8, 10, 64, 0.0), (33, 70, 256, 0.01), (64, 37, 320, 0.01),
                                          (1, 16, 4096, 0.01), (32, 1000, 512, 0.01)])
def test_fc_split_pair_bit_identical_to_fused(K, bs, Co, Ci, lam):
    """fc_recon_grad then fc_recon_apply (fed its own gv_out) against fc_recon_iter on a copy
    of the same state: loss, dL/dy, V's gradient, V, Adam's moments and the next W^ the same
    bits, over two consecutive iterations (the second reads the W^ the first carried over);
    fc_recon_grad alone leaves V, the moments and W^ as they were.  Ragged C_out tiles (10,
    37, 70), ragged batch tiles (1, 33), the smallest and largest C_in, lambda = 0."""
    s = fc_inputs(K, bs, Co, Ci, lam)
    x, tgt, w, bias, d, z = (s[k] for k in ("x", "tgt", "w", "bias", "d", "z"))
    fused = [s[k].clone() for k in ("v", "m", "s2", "what")]
    split = [s[k].clone() for k in ("v", "m", "s2", "what")]
    for k, (slot, _) in enumerate(s["slots"]):
        gv_f, gv_s = torch.empty_like(w), torch.full_like(w, float("nan"))
        loss_f, g_f = K.fc_recon_iter(x, tgt, slot, bs, w, fused[0], fused[3], d, z, 8, bias,
                                      fused[1], fused[2], 0.9, 0.999, 1e-8, gv_out=gv_f)
        before = [t.clone() for t in split]
        loss_s, g_s = K.fc_recon_grad(x, tgt, slot, bs, w, split[0], split[3], d, z, 8, bias, gv_s)
        torch.cuda.synchronize()
        for a, b, nm in zip(split, before, ("V", "exp_avg", "exp_avg_sq", "W^")):
            same_bits(a, b, f"fc_recon_grad wrote {nm} (iteration {k})")
        same_bits(loss_s, loss_f, f"loss {k}")
        same_bits(g_s, g_f, f"g {k}")
        same_bits(gv_s, gv_f, f"gV {k}")
        K.fc_recon_apply(w, split[0], split[3], d, z, 8, slot, bs, gv_s, split[1], split[2],
                         0.9, 0.999, 1e-8)
        torch.cuda.synchronize()
        for a, b, nm in zip(split, fused, ("V", "exp_avg", "exp_avg_sq", "W^")):
            same_bits(a, b, f"{nm} after iteration {k}")
        assert not torch.equal(split[0], before[0])        # the step moved V


@pytest.mark.parametrize("bs,Co,Ci", [(8, 10, 64), (33, 70, 256)])
def test_fc_apply_takes_a_foreign_gradient(K, bs, Co, Ci):
    """fc_recon_apply on a gradient that is not the kernel's own -- the sum of two different
    batches' gv_out, as the all-reduce hands back -- held in a view of a larger flat tensor
    at a 4-byte-aligned, not 16-byte-aligned offset (a bucket slice): V and the moments are
    K.adam_step's bits on that gradient, W^ is K.adaround's of the updated V."""
    s = fc_inputs(K, bs, Co, Ci, 0.01)
    w, d, z = s["w"], s["d"], s["z"]
    gvs = []
    for slot, _ in s["slots"]:
        gv = torch.empty_like(w)
        K.fc_recon_grad(s["x"], s["tgt"], slot, bs, w, s["v"], s["what"], d, z, 8, s["bias"], gv)
        gvs.append(gv)
    assert not torch.equal(gvs[0], gvs[1])
    flat = torch.zeros(Co * Ci + 7, device="cuda")
    grad = flat[3:3 + Co * Ci].view(Co, Ci)
    assert grad.data_ptr() % 16 == 12 and grad.is_contiguous()
    grad.copy_(gvs[0] + gvs[1])
    slot, words = s["slots"][0]
    v, m, s2, what = (s[k].clone() for k in ("v", "m", "s2", "what"))
    K.fc_recon_apply(w, v, what, d, z, 8, slot, bs, grad, m, s2, 0.9, 0.999, 1e-8)
    vr, mr, sr = s["v"].clone(), s["m"].clone(), s["s2"].clone()
    K.adam_step([vr], [grad.clone()], [mr], [sr], 0.9, 0.999, 1e-8,
                hyper=torch.tensor(words[2:]).cuda())
    torch.cuda.synchronize()
    for a, b, nm in ((v, vr, "V"), (m, mr, "exp_avg"), (s2, sr, "exp_avg_sq")):
        same_bits(a, b, nm)
    same_bits(what, K.adaround(v, w, d, z, 8, False, False), "W^")
    assert not torch.equal(v, s["v"])
    # the aligned read of the same gradient: the same bits
    v2, m2, s22, what2 = (s[k].clone() for k in ("v", "m", "s2", "what"))
    K.fc_recon_apply(w, v2, what2, d, z, 8, slot, bs, grad.clone(), m2, s22, 0.9, 0.999, 1e-8)
    for a, b, nm in ((v2, v, "V"), (m2, m, "exp_avg"), (s22, s2, "exp_avg_sq"), (what2, what, "W^")):
        same_bits(a, b, nm + " (16-B aligned gradient)")


def test_fc_split_loop_bit_identical_world1(Q, golden):
    """BRECQ's layer loop on the fixture's last layer (512 -> 40, batch 32, 60 iterations:
    the eager warm-up, the single-iteration graph and two chunk replays) with the split pair
    forced on (FC_SPLIT 'on': pre + post back to back, no bucket) against the fused K19 loop
    (FC_SPLIT 'off'): every recorded loss, V and Adam's moments the same bits; with the
    split on the loop calls fc_recon_grad / fc_recon_apply and never fc_recon_iter."""
    BR = importlib.import_module("shiftedscalequantization_amd.quant.block_recon")
    E = importlib.import_module("shiftedscalequantization_amd.quant._engine")
    g = golden("recon_layer_brecq_fc")
    runs = []
    for mode in ("off", "on"):
        qnn = T.build_qnn(Q, g, net=T.fc_mlp())
        fc = [m for m in qnn.modules() if isinstance(m, Q.QuantModule)][-1]
        assert tuple(fc.weight.shape) == (40, 512)
        seen, opts, calls = [], [], {"iter": 0, "grad": 0, "apply": 0}
        orig = (BR.LossFunction.record, E.SsqAdam.__init__, BR.K.fc_recon_iter,
                BR.K.fc_recon_grad, BR.K.fc_recon_apply, BR.FC_SPLIT, BR.CHUNK_ITERS)

        def spy(self, rec, rnd, b, count=None):
            seen.append(float(rec))
            return orig[0](self, rec, rnd, b, count=count)

        def init(self, *a, **k):
            orig[1](self, *a, **k)
            opts.append(self)

        def counted(name, fn):
            def f(*a, **k):
                calls[name] += 1
                return fn(*a, **k)
            return f

        (BR.LossFunction.record, E.SsqAdam.__init__, BR.K.fc_recon_iter, BR.K.fc_recon_grad,
         BR.K.fc_recon_apply, BR.FC_SPLIT, BR.CHUNK_ITERS) = (
            spy, init, counted("iter", orig[2]), counted("grad", orig[3]),
            counted("apply", orig[4]), mode, 25)
        n0 = E.GRAPH_REPLAYS.get("chunk", 0)
        try:
            assert BR.FUSE_FC, "production knobs"
            torch.manual_seed(1005)
            Q.layer_reconstruction(qnn, fc, T.dev(g["cali"]), batch_size=32, iters=60, weight=0.01,
                                   asym=True, b_range=(20, 2), warmup=0.2, act_quant=False,
                                   opt_mode="mse")
        finally:
            (BR.LossFunction.record, E.SsqAdam.__init__, BR.K.fc_recon_iter, BR.K.fc_recon_grad,
             BR.K.fc_recon_apply, BR.FC_SPLIT, BR.CHUNK_ITERS) = orig
        v = fc.weight_quantizer.alpha
        out = {"rec": np.array(seen), "V": bits(v), "m": bits(opts[0].state[v]["exp_avg"]),
               "v": bits(opts[0].state[v]["exp_avg_sq"]), "grad": bits(v.grad)}
        runs.append((out, calls, E.GRAPH_REPLAYS.get("chunk", 0) - n0))
    (off, c_off, r_off), (on, c_on, r_on) = runs
    assert c_off["iter"] >= 2 and c_off["grad"] == 0 and c_off["apply"] == 0, c_off
    assert c_on["iter"] == 0 and c_on["grad"] >= 2 and c_on["apply"] == c_on["grad"], c_on
    assert r_off >= 2 and r_on >= 2, (r_off, r_on)
    assert len(off["rec"]) == len(on["rec"]) == 60
    for k in off:
        np.testing.assert_array_equal(on[k], off[k], err_msg=k)
