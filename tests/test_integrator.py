"""The GPU path tracer as a whole against the closed form of the furnace and the float64 reference fixture: the checks of
tests/test_integrator_cpu.py (see there for what they are and why their bounds are what they are) with librt3 as the backend, over the
instance modes, the batch sizes and RT3_F_NEE_EMISSIVE, which the oracle does not have."""
import numpy as np
import pytest

import integrator_worlds as IW
from raytracer3_amd import _lib as L
from test_integrator_cpu import FURNACE_BS, LOW_CAP, check_against_fixture, check_furnace, fixture, furnace_radiance
from support import camera
from test_nee_emissive import frame, make_pt

pytestmark = pytest.mark.gpu

E = L.F_NEE_EMISSIVE
FF = L.F_FACEFORWARD
PLACEMENTS = {"world": (False, 0), "instanced_mode0": (True, 0), "instanced_mode1": (True, 1)}


def test_flag_values():
    """integrator_worlds names the flags by value, so that the fixture generator needs no built library"""
    assert (IW.F_NEE_SKY, IW.F_SPECULAR, IW.F_FACEFORWARD) == (L.F_NEE_SKY, L.F_SPECULAR, L.F_FACEFORWARD)


def furnace_pt(placement, scale=10.0):
    instanced, mode = PLACEMENTS[placement]
    mesh, inst, cam = IW.furnace(scale, instanced)
    return make_pt(mesh, IW.WINDOW_FURNACE, instances=inst, mode=mode), camera(cam, IW.WINDOW_FURNACE)


def covered(pt):
    return pt.gbuffer()[1] != L.BACKGROUND_DEPTH


# ---------------------------------------------------------------------------------------------------------------- furnace
@pytest.mark.parametrize("batch_spp", (1, 0))
@pytest.mark.parametrize("flags", (0, FF, FF | L.F_BLUENOISE))
@pytest.mark.parametrize("placement", sorted(PLACEMENTS))
def test_furnace_closed_form(placement, flags, batch_spp):
    pt, cam = furnace_pt(placement)
    try:
        pt.ctx.set_option(L.OPT_BATCH_SPP, batch_spp)
        for bounces, samples in FURNACE_BS:
            light = frame(pt, cam, flags, samples, bounces)
            low = check_furnace(light, pt.gbuffer()[0], covered(pt), bounces, samples, f"{placement} flags={flags} batch={batch_spp}")
            assert bounces > 1 or low == 0
    finally:
        pt.close()


@pytest.mark.parametrize("bounces", (2, 4))
@pytest.mark.parametrize("flags", (E, E | FF))
def test_furnace_with_emitter_sampling(flags, bounces):
    """Every triangle is an emitter.  The balance heuristic bounds each vertex's combined contribution, so a sample lies in [0, 2 L] and
    its standard deviation is at most L: the mean over all pixels and S samples lies within 5 L / sqrt(pixels x S) of L, and the leaks of
    the furnace can take at most the capped share from below.  Derived, not measured."""
    S = 1024
    pt, cam = furnace_pt("world")
    try:
        light = frame(pt, cam, flags, S, bounces).astype(np.float64)
        gb, cov = pt.gbuffer()[0], covered(pt)
        n_emitters = pt.ctx.light_info()[0]
    finally:
        pt.close()
    assert cov.all() and n_emitters == 24
    want = furnace_radiance(gb, bounces).mean((0, 1))
    ratio = light.mean((0, 1)) / want
    band = 5.0 / np.sqrt(light.shape[0] * light.shape[1] * S)
    print(f"furnace with NEE_EMISSIVE flags={flags} B={bounces}: mean / closed form {ratio}, band -{band + LOW_CAP:.4f} +{band:.4f}")
    assert np.all(ratio <= 1.0 + band) and np.all(ratio >= 1.0 - band - LOW_CAP)


# ---------------------------------------------------------------------------------------------------------------- fixture
def room_frames(name, extra_flags=0, mode=0):
    flags, bounces, specular, _, _, n_frames = IW.ROOM_CASES[name]
    pt = make_pt(IW.open_room(specular), IW.WINDOW_ROOM, sky=IW.room_sky(), mode=mode)
    try:
        cam = camera(IW.ROOM_CAMERA, IW.WINDOW_ROOM)
        frames = np.stack([frame(pt, cam, flags | extra_flags, IW.FRAME_SPP, bounces, index=k) for k in range(n_frames)])
        return frames, covered(pt)
    finally:
        pt.close()


@pytest.mark.parametrize("extra", (0, E), ids=("plain", "nee_emissive"))
@pytest.mark.parametrize("name", sorted(IW.ROOM_CASES))
def test_gpu_against_fixture(name, extra):
    frames, cov = room_frames(name, extra)
    check_against_fixture(frames, cov, fixture(), name)


def test_gpu_against_fixture_two_level():
    frames, cov = room_frames("sky_b4", mode=1)
    check_against_fixture(frames, cov, fixture(), "sky_b4")
