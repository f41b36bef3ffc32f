"""The layered BSDF and the sky sampler ON the GPU (rt3_selftest_eval ops 19-26): every evaluation is first asserted bit for bit
equal to the oracle on the same inputs, then checked against the float64 references of test_shading_math_cpu.py -- at GPU
sample counts (2^20 per case for the estimator, the visible normals and the texel histograms)."""
import numpy as np
import pytest

import orc
import ref_shading as R
import test_shading_math_cpu as S
from raytracer3_amd import _lib as L
from raytracer3_amd.render_graph import Context

pytestmark = pytest.mark.gpu
F32 = S.F32


class Device:
    """S.Oracle's interface on rt3_selftest_eval; each call asserts the oracle's answer bit for bit"""

    name = "gpu"

    def __init__(self, ctx):
        self.ctx, self.orc = ctx, S.Oracle()

    def _same(self, op, rows, out_w, ref):
        got = self.ctx.selftest(op, np.ascontiguousarray(rows, F32).view(np.uint32), out_w)
        want = np.ascontiguousarray(ref).view(np.uint32).reshape(got.shape)
        bad = np.flatnonzero((got != want).any(1))
        assert bad.size == 0, (op, bad[:4], np.asarray(rows)[bad[:4]], got[bad[:4]], want[bad[:4]])
        return got

    def bsdf_eval(self, rows):
        return self._same(19, rows, 4, orc.bsdf_eval(rows)).view(F32)

    def bsdf_sample(self, rows):
        return self._same(20, rows, 8, orc.bsdf_sample(rows))

    def sample_vndf(self, rows):
        return self._same(21, rows, 3, orc.sample_vndf(rows)).view(F32)

    def equirect_uv(self, d):
        return self._same(22, d, 2, self.orc.equirect_uv(d)).view(F32)

    def rgb9e5(self, c):
        return self._same(23, c, 1, self.orc.rgb9e5(c)[:, None]).ravel()

    def sky(self, rgb):
        return DeviceSky(self, rgb)


class DeviceSky:
    def __init__(self, dev, rgb):
        self.dev, self.ref = dev, S.OracleSky(rgb)
        dev.ctx.set_sky(rgb)
        self.shape = rgb.shape[:2]

    def tables(self):
        t = self.dev.ctx.sky_download(self.shape[1], self.shape[0])
        for a, b in zip(t, self.ref.tables()):
            assert np.array_equal(a, b)
        return t

    def sample(self, u):
        return self.dev._same(25, u, 9, self.ref.sample(u))

    def eval_pdf(self, uv):
        return self.dev._same(26, uv, 4, self.ref.eval_pdf(uv)).view(F32)


@pytest.fixture(scope="module")
def dev():
    ctx = Context(0)
    yield Device(ctx)
    ctx.close()


def test_bsdf_eval_matches_float64(dev):
    S.check_bsdf_eval(dev)
    S.check_bsdf_reciprocity(dev)


def test_bsdf_sample_is_its_own_evaluation(dev):
    S.check_bsdf_sample_consistency(dev)


def test_bsdf_sampling_is_unbiased(dev):
    """2^20 stratified samples for each of 13 (material, view) pairs, metalness 1 (p_spec = 1) and black albedo included"""
    S.check_unbiased(dev, 20)


def test_vndf_outside_the_frame_band_is_ideal(dev):
    S.check_vndf_outside_band(dev, 20)


def test_vndf_inside_the_frame_band_is_pinned(dev):
    got, asw, ideal, se = S.check_vndf_band(dev, 21)
    print(f"VNDF band (alpha 0.05, view 15 deg, 2^21 samples): mean h.x {got:.6f} +- {se:.6f}, as written {asw:.6f}, "
          f"ideal {ideal:.6f}, gap {(got - ideal) / se:.1f} standard errors")


@pytest.mark.parametrize("name", ["37x19", "5x3", "256x128", "sun1e4"])
def test_sky_sampler_matches_float64(dev, name):
    rgb = S.sky_cases()[name]
    sk = dev.sky(rgb)
    d, pdf, x, y, n_edge = S.check_sky(sk, 1 << 20, 12)
    m = n_edge + (1 << 16)
    S.check_sky_eval_roundtrip(dev, sk, d[:m], pdf[:m], x[:m], y[:m], n_edge)
    S.check_sky_seams(sk)


def test_sky_ops_need_a_sky():
    ctx = Context(0)
    for op, w in ((25, 9), (26, 4)):
        assert ctx.lib.rt3_selftest_eval(ctx.h, op, np.zeros(2, np.uint32).ctypes.data, 1, np.zeros(w, np.uint32).ctypes.data) == L.E_STATE
    ctx.close()


def test_rgb9e5_matches_float64(dev):
    """the device packer (G-buffer emissive) and the host packer of the sky texels, against each other and float64"""
    c = S.rgb9e5_inputs()
    S.check_rgb9e5(dev.rgb9e5(c), c)
    pos = c[(c >= 0).all(1) & (c <= 3.0e38).all(1)]
    sk = dev.sky(pos.reshape(1, -1, 3))
    tex = sk.tables()[1].ravel()
    assert np.array_equal(tex, dev.rgb9e5(pos))
    S.check_rgb9e5(tex, pos)
    back = dev.ctx.selftest(24, tex, 3).view(F32)
    assert np.array_equal(back.astype(np.float64), R.rgb9e5_decode(tex))
