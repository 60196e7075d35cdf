"""Golden vectors of the 2-D generators (unet_deconv / unet_vanilla with dimension=2), from the REFERENCE itself on the CPU, with the
helpers of oracle.gen_golden.

    python tools/gen_golden_unet2d.py            (from the repo root; needs the reference checkout that oracle.gen_golden names)

Writes tests/golden/unet2d_ops.npz.  Every case goes through the reference's define_G(1, 1, 64, net, norm, False, 'kaiming', 0.02, [],
dimension=2) in training mode: one forward, the loss (y * r).mean() with a seeded r, one backward.  Stored per case: state-dict keys and
shapes, parameter keys, the seeds, y and dx in full, every parameter gradient as grad_summary (l2, sum, 8 samples); for the batch-norm case
also the running statistics the step leaves and an eval() forward on them.  Weights are not stored: both sides rebuild them with
neuroclear_amd.util.seed.weights_from_seed(<spec>(2), seed)."""
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

# (tag, netG, norm, spec, input shape, weight seed)
CASES = [
    ('deconv_in_b2_16x24', 'unet_deconv', 'instance', S.unet_deconv_spec, (2, 1, 16, 24), 51),
    ('deconv_in_b1_36x20', 'unet_deconv', 'instance', S.unet_deconv_spec, (1, 1, 36, 20), 52),
    ('deconv_bn_b2_16', 'unet_deconv', 'batch', S.unet_deconv_bn_spec, (2, 1, 16, 16), 53),
    ('vanilla_in_b1_32x48', 'unet_vanilla', 'instance', S.unet_vanilla_spec, (1, 1, 32, 48), 54),
]


def gen(networks):
    out = dict(cases=np.array([c[0] for c in CASES]))
    for i, (tag, netG, norm, spec_fn, shape, seed) in enumerate(CASES):
        with contextlib.redirect_stdout(io.StringIO()):
            net = networks.define_G(1, 1, 64, netG, norm, False, 'kaiming', 0.02, [], dimension=2)
        spec = spec_fn(2)
        assert [k for k, _ in spec] == list(net.state_dict().keys()), tag
        assert [tuple(s) for _, s in spec] == [tuple(v.shape) for v in net.state_dict().values()], tag
        load_sd(net, S.weights_from_seed(spec, seed))
        net.train()
        x = torch.from_numpy(rand_input(800 + i, shape)).requires_grad_(True)
        y = net(x)
        r = torch.from_numpy(rand_input(900 + i, y.shape))
        (y * r).mean().backward()
        named = [(k, p.grad) for k, p in net.named_parameters()]
        l2, sm, samp = grad_summary(named)
        pre = tag + '_'
        out[pre + 'net'], out[pre + 'norm'], out[pre + 'seed'] = netG, norm, seed
        out[pre + 'shape'] = np.array(shape)
        out[pre + 'x_seed'], out[pre + 'r_seed'] = 800 + i, 900 + i
        out[pre + 'keys'] = np.array(list(net.state_dict().keys()))
        out[pre + 'shapes'] = np.array([','.join(str(s) for s in v.shape) for v in net.state_dict().values()])
        out[pre + 'pkeys'] = np.array([k for k, _ in named])
        out[pre + 'y'] = y.detach().numpy()
        out[pre + 'dx'] = x.grad.numpy()
        out[pre + 'g_l2'], out[pre + 'g_sum'], out[pre + 'g_samp'] = l2, sm, samp
        if norm == 'batch':
            for k, v in net.state_dict().items():
                if 'running_' in k or 'num_batches' in k:
                    out[pre + 'buf_' + k] = v.numpy().copy()
            net.eval()
            with torch.no_grad():
                out[pre + 'y_eval'] = net(torch.from_numpy(rand_input(1000 + i, shape))).numpy()
            out[pre + 'xe_seed'] = 1000 + i
        print(tag, tuple(y.shape), float(y.mean()))
    path = os.path.join(gg.OUT, 'unet2d_ops.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    gen(ref_modules())
