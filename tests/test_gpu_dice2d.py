"""GPU: the 2-D dice / assemble kernels (neuroclear_amd/csrc/dice2d.hip) and the diced inference built on them, bit for bit against the numpy
restatement (tests/dice2d_reference.py), which tests/test_dice2d_reference.py anchors to the 3-D oracle.  The entry points are called through
the C ABI with the guard buffers of tests/test_gpu_dice_geometry.py: float outputs NaN-filled between NaN guard words, integer outputs the byte
0xA5 between guards of it, so an element that is not written, or one written outside the tensor, fails.

Geometries: those of tests/test_dice2d_reference.py as stacks of 3, 2, 1, 2, 1 planes (20, 2, 192, 20, 40 tiles per plane), uint8 and uint16.
End to end: (3, 31, 40), roi 12, overlap 3, border 2 (60 tiles of 16 x 16), uint16, through unet_deconv dimension=2 and resnet_6blocks ngf 8.
Measured there on an MI355X, nbatch=8 against nbatch=1 (the share is printed, not asserted; the bound is 1 LSB): 100 % of the pixels equal through
unet_deconv, 99.81 % through resnet_6blocks, the others 1 LSB apart.  The module takes about 3 s."""
import ctypes
import functools
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dice2d_reference as D2  # noqa: E402
from oracle import dice as od  # noqa: E402
from test_dice2d_reference import GEOMS as PLANE_GEOMS, image  # noqa: E402
from test_gpu_dice_geometry import IntOut, L, Out, P, ok, stream, to_dev  # noqa: E402

from neuroclear_amd.models import networks  # noqa: E402
from neuroclear_amd.util import seed as S  # noqa: E402

DEV = 'cuda'
NC_ERR_SHAPE, NC_ERR_ARG = -1, -4
PLANES = (3, 2, 1, 2, 1)
GEOMS = [((l0,) + tuple(g[0]), g[1], g[2], g[3]) for l0, g in zip(PLANES, PLANE_GEOMS)]
IDS = ['%dx%dx%d-roi%d-ov%d-b%d' % (*g[0], g[1], g[2], g[3]) for g in GEOMS]
DTYPES = ('uint8', 'uint16')
LONG = ctypes.c_long


class Geom:
    def __init__(self, shape, roi, ov, border):
        self.L, self.roi, self.ov, self.border = tuple(shape), roi, ov, border
        self.P, self.steps = D2.geometry(shape[1:], roi, ov)
        self.per = self.steps[0] * self.steps[1]
        self.n = shape[0] * self.per
        self.E = roi + 2 * border
        self.nacc = shape[0] * self.P[0] * self.P[1]


@functools.lru_cache(maxsize=None)
def reference(gi, dtype):
    """per geometry and type, computed once: the stack, its tiles, random tiles, their accumulator and finalised stack, the round trip"""
    g = Geom(*GEOMS[gi])
    stack = image(g.L, dtype, 300 + gi)
    tiles = D2.tiles2d(stack, g.roi, g.ov, g.border)
    rand = (0.99 * np.random.default_rng(400 + gi).random((g.n, g.E, g.E))).astype(np.float32)
    acc = D2.assemble2d(rand, g.L, g.roi, g.ov, g.border)
    out = D2.finalize2d(acc, g.L, g.roi, g.ov, dtype)
    back = D2.finalize2d(D2.assemble2d(tiles, g.L, g.roi, g.ov, g.border), g.L, g.roi, g.ov, dtype)
    for a in (stack, tiles, rand, acc, out, back):
        a.setflags(write=False)
    return g, stack, tiles, rand, acc, out, back


def dev_cut(g, vd, u16, batch):
    tiles = Out(g.n * g.E * g.E)
    for first in range(0, g.n, batch):
        count = min(batch, g.n - first)
        ok(L().nc_dice2d_cut_tiles(P(vd), u16, g.L[0], g.L[1], g.L[2], g.roi, g.ov, g.border, LONG(first), count, P(tiles.t[first * g.E * g.E:]), stream()),
           'nc_dice2d_cut_tiles')
    assert tiles.intact()
    return tiles


def dev_accumulate(g, td, batch):
    acc = Out(g.nacc, np.zeros(g.nacc, np.float32))
    for first in range(0, g.n, batch):
        count = min(batch, g.n - first)
        ok(L().nc_assemble2d_scatter_add(P(td.view(-1)[first * g.E * g.E:]), P(acc.t), g.L[0], g.P[0], g.P[1], g.roi, g.ov, g.border, LONG(first), count,
                                         stream()), 'nc_assemble2d_scatter_add')
    assert acc.intact()
    return acc


def dev_finalize(g, acc, dtype):
    out = IntOut(g.L[0] * g.L[1] * g.L[2], dtype)
    ok(L().nc_assemble2d_finalize(P(acc.t), P(out.t), int(dtype == 'uint16'), g.L[0], g.P[0], g.P[1], g.L[1], g.L[2], g.roi, g.ov, stream()),
       'nc_assemble2d_finalize')
    assert out.intact()
    return out


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('gi', range(len(GEOMS)), ids=IDS)
def test_cut_tiles_bit_exact(gi, dtype):
    g, stack, want, *_ = reference(gi, dtype)
    assert want.shape == (g.n, g.E, g.E)
    vd = to_dev(stack)
    for batch in (g.n, 1, 7):     # all tiles in one call; one per call; batches of 7 (they straddle planes at 20 tiles per plane)
        got = dev_cut(g, vd, int(dtype == 'uint16'), batch).bits().reshape(want.shape)
        bad = np.nonzero((got != want.view(np.int32)).reshape(g.n, -1).any(1))[0]
        assert bad.size == 0, ('batch', batch, 'tiles that differ', bad[:10])
    if gi == 0:
        assert g.per == 20 and g.n == 60     # the batch [14, 21) holds tiles of planes 0 and 1


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('gi', range(len(GEOMS)), ids=IDS)
def test_scatter_add_and_finalize_bit_exact(gi, dtype):
    g, _, _, rand, acc_np, out_np, _ = reference(gi, dtype)
    td = to_dev(rand.copy())
    for batch in (1, 3, 7, g.n):
        acc = dev_accumulate(g, td, batch)
        assert np.array_equal(acc.bits(), acc_np.view(np.int32).reshape(-1)), ('batch', batch)
    out = dev_finalize(g, acc, dtype)
    assert np.array_equal(out.array(g.L), out_np)
    # an accumulator of all-ones tiles finalises to the top of the type
    ones = dev_finalize(g, dev_accumulate(g, torch.ones(g.n * g.E * g.E, device=DEV), 5), dtype)
    assert bool((ones.array(g.L) == np.iinfo(dtype).max).all())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('gi', range(len(GEOMS)), ids=IDS)
def test_round_trip(gi, dtype):
    """dice -> assemble of the input on the device: the restatement's round trip exactly, the input within 1 LSB"""
    g, stack, _, _, _, _, back = reference(gi, dtype)
    tiles = dev_cut(g, to_dev(stack), int(dtype == 'uint16'), 7)
    got = dev_finalize(g, dev_accumulate(g, tiles.t, 7), dtype).array(g.L)
    assert np.array_equal(got, back)
    assert int(np.abs(got.astype(np.int64) - stack.astype(np.int64)).max()) <= 1


def test_refused_geometries_leave_the_outputs_untouched():
    g, stack, *_ = reference(0, 'uint16')     # (3, 31, 40), roi 12, overlap 3, border 2: padded 39 x 48, 60 tiles
    vd = to_dev(stack)
    tiles, acc, out = Out(g.n * g.E * g.E), Out(g.nacc), IntOut(g.L[0] * g.L[1] * g.L[2], 'uint16')
    src, zero = torch.ones(g.n * g.E * g.E, device=DEV), torch.zeros(g.nacc, device=DEV)
    st = stream()
    cut = lambda roi, ov, b, first, count: L().nc_dice2d_cut_tiles(P(vd), 1, g.L[0], g.L[1], g.L[2], roi, ov, b, LONG(first), count, P(tiles.t), st)  # noqa: E731
    sca = lambda roi, ov, b, first, count, Ps=g.P: L().nc_assemble2d_scatter_add(P(src), P(acc.t), g.L[0], Ps[0], Ps[1], roi, ov, b, LONG(first), count, st)  # noqa: E731
    fin = lambda Ps, roi, ov: L().nc_assemble2d_finalize(P(zero), P(out.t), 1, g.L[0], Ps[0], Ps[1], g.L[1], g.L[2], roi, ov, st)  # noqa: E731
    # roi <= overlap
    for ov in (12, 13):
        assert cut(12, ov, 2, 0, 1) == NC_ERR_SHAPE and sca(12, ov, 2, 0, 1) == NC_ERR_SHAPE and fin(g.P, 12, ov) == NC_ERR_SHAPE
    # overlap 0: the reference assembler adds nothing then
    assert sca(12, 0, 2, 0, 1) == NC_ERR_SHAPE and fin(g.P, 12, 0) == NC_ERR_SHAPE
    # no border, and a border of the smaller padded length or more (np.pad's reflect would fold twice)
    assert cut(12, 3, 0, 0, 1) == NC_ERR_SHAPE and sca(12, 3, 0, 0, 1) == NC_ERR_SHAPE
    assert cut(12, 3, min(g.P), 0, 1) == NC_ERR_SHAPE and cut(12, 3, min(g.P) + 5, 0, 1) == NC_ERR_SHAPE
    assert sca(12, 3, min(g.P), 0, 1) == NC_ERR_SHAPE
    # first < 0, count < 1, first + count > the number of tiles
    for first, count in ((-1, 1), (0, 0), (0, -1), (g.n, 1), (g.n - 6, 7), (0, g.n + 1)):
        assert cut(12, 3, 2, first, count) == NC_ERR_SHAPE, (first, count)
        assert sca(12, 3, 2, first, count) == NC_ERR_SHAPE, (first, count)
    # a padded size that is not pad_for_dicing of the original size
    for k in range(2):
        for d in (1, -1):
            assert fin(tuple(p + d * (i == k) for i, p in enumerate(g.P)), 12, 3) == NC_ERR_SHAPE
    # null pointers
    assert L().nc_dice2d_cut_tiles(P(None), 1, g.L[0], g.L[1], g.L[2], 12, 3, 2, LONG(0), 1, P(tiles.t), st) == NC_ERR_ARG
    assert L().nc_dice2d_cut_tiles(P(vd), 1, g.L[0], g.L[1], g.L[2], 12, 3, 2, LONG(0), 1, P(None), st) == NC_ERR_ARG
    assert L().nc_assemble2d_scatter_add(P(src), P(None), g.L[0], g.P[0], g.P[1], 12, 3, 2, LONG(0), 1, st) == NC_ERR_ARG
    assert L().nc_assemble2d_finalize(P(zero), P(None), 1, g.L[0], g.P[0], g.P[1], g.L[1], g.L[2], 12, 3, st) == NC_ERR_ARG
    torch.cuda.synchronize()
    assert tiles.untouched() and acc.untouched() and out.untouched()
    # ... and the same calls with good arguments go through (the last border accepted, the last tiles)
    assert cut(12, 3, 2, g.n - 7, 7) == 0 and sca(12, 3, 2, g.n - 7, 7) == 0 and fin(g.P, 12, 3) == 0
    torch.cuda.synchronize()


# ---- end to end: (3, 31, 40), roi 12, overlap 3, border 2, uint16

def make_opt(**kw):
    g = Geom(*GEOMS[0])
    opt = Namespace(dice_size=[g.roi] * 2, overlap=g.ov, border_cut=g.border, gpu_ids=[0], skip_real=True, data_type='uint16', histogram_match=False,
                    normalize_intensity=False)
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def make_net(name):
    if name == 'unet_deconv':
        net = networks.define_G(1, 1, 64, 'unet_deconv', 'instance', False, 'kaiming', 0.02, [0], dimension=2)
        net.load_state_dict(S.state_dict_from_seed(S.unet_deconv_spec(2), 71, DEV))
    else:
        net = networks.define_G(1, 1, 8, 'resnet_6blocks', 'instance', False, 'kaiming', 0.02, [0], dimension=2)
        net.load_state_dict(S.state_dict_from_seed(S.resnet_spec(6, 8), 72, DEV))
    return net


@pytest.fixture(scope='module', params=['unet_deconv', 'resnet_6blocks'])
def e2e(request):
    """the net, and its output for every restated tile, one tile per call"""
    g, stack, tiles, *_ = reference(0, 'uint16')
    net = make_net(request.param)
    with torch.no_grad():
        outs = np.stack([net(torch.from_numpy(tiles[t].copy())[None, None].to(DEV))[0, 0].cpu().numpy() for t in range(g.n)])
    assert outs.shape == tiles.shape and 0.0 <= float(outs.min()) and float(outs.max()) < 1.0 and float(outs.std()) > 0.0
    want = D2.finalize2d(D2.assemble2d(outs, g.L, g.roi, g.ov, g.border), g.L, g.roi, g.ov, 'uint16')
    return request.param, net, outs, want


def test_diced_inference_2d_against_the_restatement(e2e):
    from neuroclear_amd.infer_dice2d import diced_inference_2d
    name, net, _, want = e2e
    g, stack, _, _, _, _, back = reference(0, 'uint16')
    one = diced_inference_2d(net, stack, make_opt(), nbatch=1)
    assert one.shape == want.shape == g.L and one.dtype == np.uint16
    assert np.array_equal(one, want)
    calls = []
    eight, real = diced_inference_2d(net, stack, make_opt(), nbatch=8, with_real=True, on_batch=lambda fn: (calls.append(1), fn())[1])
    assert len(calls) == (g.n + 7) // 8
    d = np.abs(eight.astype(np.int64) - one.astype(np.int64))
    print('%s: nbatch 8 against nbatch 1: %.4f %% of the pixels equal, max |diff| %d LSB' % (name, 100.0 * float((d == 0).mean()), int(d.max())))
    assert int(d.max()) <= 1     # batch mates change fp32 rounding of the InstanceNorm statistics only
    assert real.shape == g.L and np.array_equal(real, back)
    # one plane: the same bits, and a 2-D result
    plane = diced_inference_2d(net, stack[1], make_opt(), nbatch=1)
    assert plane.shape == g.L[1:] and np.array_equal(plane, one[1])


def test_diced_inference_2d_with_histogram_match(e2e):
    """every output tile's R x R interior matched to its input tile's interior by the oracle, then assembled: <= 1 LSB, the bound of
    tests/test_histmatch.py's end-to-end test (the device rounds the float64 match to float32 before it is added)"""
    from neuroclear_amd.infer_dice2d import diced_inference_2d
    _, net, outs, _ = e2e
    g, stack, tiles, *_ = reference(0, 'uint16')
    b = g.border
    matched = outs.copy()
    for t in range(g.n):
        matched[t, b:-b, b:-b] = od.match_histograms_np(outs[t, b:-b, b:-b], tiles[t, b:-b, b:-b]).astype(np.float32)
    want = D2.finalize2d(D2.assemble2d(matched, g.L, g.roi, g.ov, g.border), g.L, g.roi, g.ov, 'uint16')
    got = diced_inference_2d(net, stack, make_opt(histogram_match=True), nbatch=1)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max()) <= 1
    assert not np.array_equal(got, e2e[3])


def test_classes_mirror_the_3d_ones():
    from neuroclear_amd.data.diceImage2d_dataset import DiceImage2DDataSet
    from neuroclear_amd.util.assemble_dice2d import Assemble_Dice2D
    g, stack, tiles, _, _, _, back = reference(0, 'uint16')
    opt = make_opt(skip_real=False)
    ds = DiceImage2DDataSet(opt, image=stack)
    assert len(ds) == g.n and ds.size_original() == g.L and ds.size() == (g.L[0],) + g.P and ds.shape() == (g.L[0],) + g.steps
    item = ds[g.n - 1]
    assert item['A_paths'] == str(g.n - 1) and tuple(item['A'].shape) == (1, g.E, g.E)
    assert np.array_equal(item['A'][0].cpu().numpy().view(np.int32), tiles[g.n - 1].view(np.int32))
    assert tuple(ds.cut(3, 9).shape) == (9, 1, g.E, g.E)
    with pytest.raises(IndexError):
        ds[g.n]
    with pytest.raises(ValueError, match='border_cut must be >= 1'):
        DiceImage2DDataSet(make_opt(border_cut=0), image=stack)
    with pytest.raises(TypeError, match='must be uint8 or uint16'):
        DiceImage2DDataSet(opt, image=stack.astype(np.float32))
    with pytest.raises(ValueError):
        DiceImage2DDataSet(opt, image=stack[None])
    asm = Assemble_Dice2D(opt, g.L)
    for t in range(g.n - 1):     # one tile per call, in index order, as the 3-D class takes them
        x = ds[t]['A'].unsqueeze(0)
        asm.addToStack({'real': x, 'fake': x})
    with pytest.raises(Exception, match='expected %d tiles' % g.n):
        asm.assemble_all()
    x = ds[g.n - 1]['A'].unsqueeze(0)
    asm.addToStack({'real': x, 'fake': x})
    asm.assemble_all()
    out = asm.getDict()
    assert list(out) == ['real', 'fake'] and out['fake'].dtype == np.uint16
    assert np.array_equal(out['fake'], back) and np.array_equal(out['real'], back)
    # add_tiles alone counts its tiles: a batch short raises, the complete sequence finalises
    asm = Assemble_Dice2D(make_opt(), g.L)
    asm.add_tiles('fake', ds.cut(0, g.n - 5), 0)
    with pytest.raises(Exception, match='expected %d tiles for fake, got %d' % (g.n, g.n - 5)):
        asm.assemble_all()
    asm.add_tiles('fake', ds.cut(g.n - 5, 5), g.n - 5)
    asm.assemble_all()
    assert list(asm.getDict()) == ['fake'] and np.array_equal(asm.getDict()['fake'], back)


def test_both_datasets_load_their_input_alike():
    """One loader behind both classes (data/diceImage_dataset.load_resident): a torch tensor that is neither uint8, int16 nor uint16 is refused
    -- the 3-D class used to read it as uint8 --, a read-only numpy array is copied, and int16 / uint16 tensors carry uint16 bits."""
    from neuroclear_amd.data.diceImage2d_dataset import DiceImage2DDataSet
    from neuroclear_amd.data.diceImage_dataset import DiceImageDataSet
    g, stack, tiles, *_ = reference(0, 'uint16')
    assert not stack.flags.writeable
    opt = make_opt()
    signed = torch.from_numpy(stack.view(np.int16).copy())
    for cls in (DiceImageDataSet, DiceImage2DDataSet):
        for dt in (torch.float32, torch.int32, torch.int8, torch.float16):
            with pytest.raises(TypeError, match='must be uint8 or uint16'):
                cls(opt, signed.to(dt))
        with pytest.raises(TypeError, match='must be uint8 or uint16'):
            cls(opt, stack.astype(np.int16))
        resident = [cls(opt, stack), cls(opt, signed), cls(opt, signed.to(DEV))]
        assert all(d.is_u16 and d.size_original() == g.L for d in resident)
        assert not cls(opt, stack.astype(np.uint8)).is_u16 and not cls(opt, signed.to(torch.uint8)).is_u16
        first = [d[0]['A'].cpu().numpy() for d in resident]
        assert np.array_equal(first[0], first[1]) and np.array_equal(first[0], first[2])
    # the 2-D set's first tile is the restatement's; the 3-D set's first cube holds the same pixels where the two overlap (plane 0, no reflection)
    assert np.array_equal(first[0][0].view(np.int32), tiles[0].view(np.int32))
    cube = DiceImageDataSet(opt, stack)[0]['A'][0].cpu().numpy()
    b = g.border
    assert np.array_equal(cube[b, b:, b:].view(np.int32), tiles[0][b:, b:].view(np.int32))


@pytest.mark.parametrize('ndim', [2, 3])
def test_main_with_image_dimension_2(tmp_path, ndim):
    """A seeded checkpoint saved under the reference's file name; the 2-D entry script (neuroclear_amd.infer_dice2d.main, test_dice.py's command
    line with --image_dimension 2) runs a .npy plane and a .npy stack through diced_inference_2d and writes volumes/output_volume.npy as the 3-D
    path does (a plane as a stack of one)."""
    from neuroclear_amd.infer_dice2d import diced_inference_2d, main
    g, stack, *_ = reference(0, 'uint16')
    img = stack if ndim == 3 else stack[2]
    ck, data, res = tmp_path / 'ckpt', tmp_path / 'data', tmp_path / 'results'
    (ck / 'm').mkdir(parents=True)
    data.mkdir()
    np.save(str(data / 'image.npy'), img)
    spec = S.resnet_spec(6, 8)
    torch.save(S.state_dict_from_seed(spec, 72), str(ck / 'm' / 'iter_3_net_G.pth'))
    argv = ['--dataroot', str(data), '--checkpoints_dir', str(ck), '--results_dir', str(res), '--name', 'm', '--netG', 'resnet_6blocks', '--ngf', '8',
            '--norm', 'instance', '--image_dimension', '2', '--load_iter', '3', '--gpu_ids', '0', '--no_dropout', '--dice_size', '12', '12',
            '--overlap', '3', '--border_cut', '2', '--data_type', 'uint16', '--skip_real']
    main(argv)
    got = np.load(str(res / 'm' / 'test_latest_iter3' / 'volumes' / 'output_volume.npy'))
    want = diced_inference_2d(make_net('resnet_6blocks'), img, make_opt())
    assert want.shape == img.shape
    assert got.dtype == np.uint16 and got.shape == ((1,) + img.shape if ndim == 2 else img.shape)
    assert np.array_equal(got.reshape(img.shape), want) and int(want.max()) > int(want.min())
    if ndim == 2:
        with pytest.raises(NotImplementedError, match='normalize_intensity'):
            main(argv + ['--normalize_intensity'])
        with pytest.raises(NotImplementedError, match='image_dimension 3'):
            main(argv[:argv.index('--image_dimension')] + ['--image_dimension', '3'] + argv[argv.index('--image_dimension') + 2:])
