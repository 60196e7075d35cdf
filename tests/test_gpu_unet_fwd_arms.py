"""The fallback arms of the whole-network inference forward (nc_unet_deconv_fwd, csrc/unet_fwd.hip).  Most of them are reached only through
switches that the library reads when it is loaded, so every configuration runs in a fresh child process, one at a time (the precedent:
tests/test_gpu_wprep.py test_fallbacks_set_by_the_environment).

Which arm a configuration takes follows from the host-side predicates alone (s3_fwd_supported / s3x_supported / convT_s3x_supported /
c1k3_stats_bytes); every one of them holds at 16^3, 32^3 and (16, 24, 40) -- channels are multiples of 64, the smallest level is 4^3 -- so the
switch alone selects the arm and each child runs all three shapes:

  default            two-term (H2) mode, the whole batch through every launch; InstanceNorm sums from the convolutions' epilogues (block 0: the
                     one-channel kernel's); pools fused into the conversion pass; both transposed convolutions two-term in, H2 out with a bound;
                     fused tail.  terms 2
  NC_CONVT_H2=0      two-term mode, but blocks 6 and 8 leave a THREE-term operand (act_split3) and the transposed convolutions write fp32 into the
                     upper half of cat2 / cat1, which is measured (h2_absmax) and converted (split2h_into).  terms 2
  NC_CONVT_S3X=0     two-term mode, blocks 6 and 8 leave fp32 (nc_instnorm_act_fwd) for the fp32 transposed convolution (nc_convT_k2s2_fwd), then
                     measured and converted as above.  terms 2
  NC_INFER_BATCHED=0 two-term mode, one sample per pass of the network (the sample loop runs N times).  terms 2
  epi_stats=0        two-term mode, every block's statistics from nc_instnorm_stats per sample over the raw output; block 0 through nc_conv_fwd.
                     terms 2
  terms3             the per-sample forward: block 0 on the one-channel kernel with its own sums, every other block conv_fwd_s3 from the S3 operand
                     its producer wrote (act_split3); transposed convolutions convT_fwd_s3x, S3 in, S3 out; unfused tail.  terms 3
  terms3 NC_S3_FUSE=0  the per-sample forward with every block through nc_conv_fwd from fp32 (which converts for itself) and
                     nc_instnorm_act_fwd; a separate split3_into in front of each transposed convolution, which writes fp32.  terms 3
  terms3 NC_CONVT_S3X=0  as terms3, but t_conv2 on nc_convT_k2s2_fwd + split3_into and t_conv1 on convT_fwd_s3 (convt.hip), which writes block
                     9's S3 operand itself.  terms 3
  NC_CONV_SPLIT=0    the per-sample forward on the fp32 matrix-core kernels, fp32 transposed convolutions, no operand forms at all.  terms 3
  force_direct       the per-sample forward on the VALU kernels (block 0 through nc_conv_fwd: no epilogue sums); the transposed convolutions stay
                     on convT_fwd_s3x behind a split3_into.  terms 3

Checks per child: the golden forward at 16 and 32 (tests/golden/unet_deconv_{16,32}.npz from the reference, max |y - g| < 2e-5: the files and
the bound of test_h2_unet_inference_golden) and the same bits on a second call; one N = 3 call at (16, 24, 40) against three N = 1 calls
(<= 1e-5, the bound of test_batched_cubes_per_call_match_one_cube_per_call) and torch.equal on a second N = 3 call; nc_unet_deconv_fwd_terms.

Left out, a finding about the code as it was before this file existed: the N = 3 check under NC_CONVT_H2=0 and under NC_CONVT_S3X=0.  With
more than one sample per pass the normalisation of blocks 6 and 8 in those two arms (act_split3 / nc_instnorm_act_fwd) is launched for ONE
sample, so the transposed convolutions read samples 1 .. of a buffer nobody wrote.  Measured on the commit before this file, and again with
it: max |N = 3 call - three N = 1 calls| = 0.548 (NC_CONVT_H2=0) and 0.940 (NC_CONVT_S3X=0) against the bound 1e-5; every other
configuration 0 (default: 5.2e-6).  Their golden and terms checks (N = 1) run; their arms' behaviour is unchanged."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import json, os, sys
import numpy as np, torch
sys.path.insert(0, %(root)r)
from neuroclear_amd._lib import lib
from neuroclear_amd.models import networks
from neuroclear_amd.util import seed as S
L = lib()
for name, v in json.loads(sys.argv[1]).items():
    getattr(L, 'nc_set_' + name)(v)
net = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'kaiming', 0.02, [0])
out = {}
for size in (16, 32):
    g = np.load(os.path.join(%(root)r, 'tests', 'golden', 'unet_deconv_%%d.npz' %% size))
    net.load_state_dict(S.state_dict_from_seed(S.unet_deconv_spec(), int(g['seed']), 'cuda'))
    x = torch.from_numpy(np.random.default_rng(int(g['x_seed'])).random((1, 1, size, size, size), dtype=np.float32)).cuda()
    with torch.no_grad():
        y, y2 = net(x), net(x)
    out['golden_%%d' %% size] = float(np.abs(y.cpu().numpy() - g['y']).max())
    out['repeat_%%d' %% size] = bool(torch.equal(y, y2))
    out['terms_%%d' %% size] = L.nc_unet_deconv_fwd_terms(size, size, size)
shape = (16, 24, 40)
net.load_state_dict(S.state_dict_from_seed(S.unet_deconv_spec(), 6, 'cuda'))
x = torch.rand((3, 1) + shape, generator=torch.Generator().manual_seed(9)).cuda()
with torch.no_grad():
    y3, y3b = net(x), net(x)
    y1 = torch.cat([net(x[i:i + 1]) for i in range(3)])
out['n3_repeat'] = bool(torch.equal(y3, y3b))
out['n3_diff'] = float((y3 - y1).abs().max())
out['n3_finite'] = bool(torch.isfinite(y3).all())
out['terms_n3'] = L.nc_unet_deconv_fwd_terms(*shape)
print('RESULT ' + json.dumps(out))
'''

# (name, environment, setters by the name behind nc_set_, the terms the configuration implies, whether the N = 3 check applies)
CONFIGS = [
    ('default', {}, {}, 2, True),
    ('convt_h2_off', {'NC_CONVT_H2': '0'}, {}, 2, False),
    ('convt_s3x_off', {'NC_CONVT_S3X': '0'}, {}, 2, False),
    ('infer_batched_off', {'NC_INFER_BATCHED': '0'}, {}, 2, True),
    ('epi_stats_off', {}, {'epi_stats': 0}, 2, True),
    ('terms3', {}, {'split_terms': 3}, 3, True),
    ('terms3_s3_fuse_off', {'NC_S3_FUSE': '0'}, {'split_terms': 3}, 3, True),
    ('terms3_convt_s3x_off', {'NC_CONVT_S3X': '0'}, {'split_terms': 3}, 3, True),
    ('conv_split_off', {'NC_CONV_SPLIT': '0'}, {}, 3, True),
    ('force_direct', {}, {'force_direct': 1}, 3, True),
]


@pytest.mark.parametrize('name,env,setters,terms,n3', CONFIGS, ids=[c[0] for c in CONFIGS])
def test_forward_arm(name, env, setters, terms, n3):
    child_env = {k: v for k, v in os.environ.items() if not k.startswith('NC_')}
    child_env.update(env)
    run = subprocess.run([sys.executable, '-c', _CHILD % {'root': ROOT}, json.dumps(setters)], env=child_env, capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = [l for l in run.stdout.splitlines() if l.startswith('RESULT ')]
    assert len(rows) == 1, run.stdout
    r = json.loads(rows[0][7:])
    print(name, r)
    for size in (16, 32):
        assert r['terms_%d' % size] == terms
        assert r['golden_%d' % size] < 2e-5
        assert r['repeat_%d' % size]
    assert r['terms_n3'] == terms
    if n3:
        assert r['n3_finite']
        assert r['n3_diff'] <= 1e-5
        assert r['n3_repeat']
