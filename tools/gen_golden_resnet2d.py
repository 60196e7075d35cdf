"""Golden vectors of the ResNet generators (resnet_6blocks / resnet_9blocks, dimension=2), from the REFERENCE itself on the CPU, with the helpers
of oracle.gen_golden.

    python tools/gen_golden_resnet2d.py            (from the repo root; needs the reference checkout that oracle.gen_golden names)

Writes tests/golden/resnet2d_ops.npz.  Every case goes through the reference's define_G(1, 1, ngf, net, norm, use_dropout, 'kaiming', 0.02, [],
dimension=2): one forward, the loss (y * r).mean() with a seeded r -- y.mean() where the output shape differs from the input's -- and one
backward; in training mode, or in eval() for the dropout case (Dropout is the identity there).  Stored per case: state-dict keys and shapes,
parameter keys, the seeds, y and dx in full, every parameter gradient as grad_summary (l2, sum, 8 samples); for the batch-norm case also the
running statistics the step leaves and an eval() forward on them.  The same step is repeated on net.double(): `_d64` holds the reference's own
float32-to-float64 distances (|y| max, dx relative L2, worst parameter-gradient |l2 difference| / (l2 + 1e-6 / 2e-2)), which must use at most a
third of the bounds the GPU tests apply (2e-5, 2e-2, 2e-2).  Weights are not stored: both sides rebuild them with
neuroclear_amd.util.seed.weights_from_seed(resnet_spec(...), seed)."""
import contextlib
import io
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from oracle import gen_golden as gg  # noqa: E402
from oracle.gen_golden import grad_summary, load_sd, rand_input, ref_modules  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402

# (tag, netG, n_blocks, norm, ngf, use_dropout, eval mode, input shape, weight seed)
CASES = [
    ('r6_in_ngf16_b2_32x40', 'resnet_6blocks', 6, 'instance', 16, False, False, (2, 1, 32, 40), 71),
    ('r9_in_ngf8_b1_36x28', 'resnet_9blocks', 9, 'instance', 8, False, False, (1, 1, 36, 28), 72),
    ('r6_bn_ngf8_b2_24', 'resnet_6blocks', 6, 'batch', 8, False, False, (2, 1, 24, 24), 73),
    ('r6_in_drop_eval_30x22', 'resnet_6blocks', 6, 'instance', 8, True, True, (1, 1, 30, 22), 74),
]
BOUNDS = (2e-5, 2e-2, 2e-2)


def step(net, x_np, r_seed, dtype):
    x = torch.from_numpy(x_np).to(dtype).requires_grad_(True)
    y = net(x)
    if tuple(y.shape) == tuple(x.shape):
        (y * torch.from_numpy(rand_input(r_seed, y.shape)).to(dtype)).mean().backward()
    else:
        y.mean().backward()
    return y.detach(), x.grad, [(k, p.grad) for k, p in net.named_parameters()]


def rel2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def gen(networks):
    out = dict(cases=np.array([c[0] for c in CASES]))
    for i, (tag, netG, nb, norm, ngf, drop, ev, shape, seed) in enumerate(CASES):
        spec = S.resnet_spec(nb, ngf, 1, 1, norm, drop)

        def build(dtype):
            with contextlib.redirect_stdout(io.StringIO()):
                net = networks.define_G(1, 1, ngf, netG, norm, drop, 'kaiming', 0.02, [], dimension=2)
            assert [k for k, _ in spec] == list(net.state_dict().keys()), tag
            assert [tuple(s) for _, s in spec] == [tuple(v.shape) for v in net.state_dict().values()], tag
            load_sd(net, S.weights_from_seed(spec, seed))
            net = net.to(dtype)
            return net.eval() if ev else net.train()

        x_np = rand_input(1100 + i, shape)
        net = build(torch.float32)
        y, dx, named = step(net, x_np, 1200 + i, torch.float32)
        y64, dx64, named64 = step(build(torch.float64), x_np, 1200 + i, torch.float64)
        l2, sm, samp = grad_summary(named)
        l264 = np.array([float(g.double().pow(2).sum().sqrt()) for _, g in named64])
        d64 = np.array([float((y.double() - y64).abs().max()), rel2(dx.numpy(), dx64.numpy()),
                        float(np.max(np.abs(l2 - l264) / (l264 + 1e-6 / 2e-2)))])
        assert all(d <= b / 3 for d, b in zip(d64, BOUNDS)), (tag, d64)
        pre = tag + '_'
        out[pre + 'net'], out[pre + 'norm'], out[pre + 'seed'], out[pre + 'ngf'] = netG, norm, seed, ngf
        out[pre + 'n_blocks'], out[pre + 'dropout'], out[pre + 'eval'] = nb, int(drop), int(ev)
        out[pre + 'shape'], out[pre + 'yshape'] = np.array(shape), np.array(y.shape)
        out[pre + 'x_seed'], out[pre + 'r_seed'] = 1100 + i, 1200 + i
        out[pre + 'keys'] = np.array(list(net.state_dict().keys()))
        out[pre + 'shapes'] = np.array([','.join(str(s) for s in v.shape) for v in net.state_dict().values()])
        out[pre + 'pkeys'] = np.array([k for k, _ in named])
        out[pre + 'y'] = y.numpy()
        out[pre + 'dx'] = dx.numpy()
        out[pre + 'g_l2'], out[pre + 'g_sum'], out[pre + 'g_samp'] = l2, sm, samp
        out[pre + 'd64'] = d64
        if norm == 'batch':
            for k, v in net.state_dict().items():
                if 'running_' in k or 'num_batches' in k:
                    out[pre + 'buf_' + k] = v.numpy().copy()
            net.eval()
            with torch.no_grad():
                out[pre + 'y_eval'] = net(torch.from_numpy(rand_input(1300 + i, shape))).numpy()
            out[pre + 'xe_seed'] = 1300 + i
        print(tag, tuple(y.shape), float(y.mean()), 'fp32 - fp64: y %.2e dx %.2e grads %.2e' % tuple(d64))
    path = os.path.join(gg.OUT, 'resnet2d_ops.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    gen(ref_modules())
