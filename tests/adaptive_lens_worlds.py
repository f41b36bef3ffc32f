"""The frames the coverage-mode tests of the "adaptive" pass share (rt3_adaptive_set_coverage, DESIGN.md section 4l:
tests/test_adaptive_lens_cpu.py, tests/test_adaptive_lens.py).

World A: the fixture of tests/adaptive_worlds.py (scenes.cornell() seen from outside, 67 x 45: no multiple of 64 or 256, two tiles of the
partition; its 3015 list entries make two 2048-entry compaction blocks, which is all of the compaction these frames exercise: the scan's
wave and chunk boundaries are tests/test_adaptive_compaction.py's) through a thin lens focused on the wall the camera faces.
With a lens every pixel is listed: the background around the wall is the small sky, antialiased along the wall's outline.
World B: glass_worlds.glass_room() (a solid glass block and a thin-walled pane in integrator_worlds' open room) at glass_worlds' 64 x 48
window under the antialiasing pinhole, four bounces.
min_samples = step = 4 and cap 24 as in adaptive_worlds.

THRESHOLD[world][dilate] was picked on predictions, not on what the pass does: "refrence_mode" frames with the world's lens at samples =
1 .. CAP (kernels the coverage mode does not change), per-sample luminances rebuilt from them in float64 as k m_k - (k - 1) m_(k-1)
(test_adaptive.test_moments_against_float64 has the error bound), and ref_adaptive.simulate over them with every pixel foreground.  The
shares it predicted (stopping before the cap, reaching it), each wanted at 0.25 or more so that the pass's own bits -- which are not the
rebuilt samples' -- still clear adaptive_worlds.MIN_SHARE = 0.15:
    A, dilate 0: threshold 0.08 -> 0.588 / 0.412        A, dilate 1: threshold 0.12 -> 0.529 / 0.471
    B, dilate 0: threshold 0.10 -> 0.498 / 0.502        B, dilate 1: threshold 0.15 -> 0.411 / 0.589
(In A a little over half of the window is the small sky around the wall, smooth enough to stop under any of the thresholds tried; the wall
decides the rest.)
test_adaptive_lens.test_thresholds_were_picked_on_predictions renders the prediction again and asserts the 0.25."""
import adaptive_worlds as aw
import glass_worlds as GW
import integrator_worlds as IW

MIN_SAMPLES, STEP, CAP, DARK, FRAME = aw.MIN_SAMPLES, aw.STEP, aw.CAP, aw.DARK, aw.FRAME
CAPS = list(range(MIN_SAMPLES, CAP + 1, STEP))  # 4, 8, ..., 24
PREDICTED_SHARE = 0.25

F_NEE_SKY, F_FACEFORWARD, F_NEE_EMISSIVE = 1, 8, 32  # RT3_F_* of include/rt3.h

# name -> what a frame of the world is made of
A = dict(name="A", window=(aw.W, aw.H), camera=aw.CAMERA, lens=(0.05, 3.5, 1.0),  # the wall (z = 4) is 3.5 in front of the eye (z = 7.5)
         bounces=aw.BOUNCES, flags=aw.FLAGS, threshold={0: 0.08, 1: 0.12})
B = dict(name="B", window=GW.WINDOW, camera=IW.ROOM_CAMERA, lens=GW.ROOM_LENS, bounces=4, flags=F_NEE_SKY | F_FACEFORWARD | F_NEE_EMISSIVE,
         threshold={0: 0.10, 1: 0.15})


def params(world, **kw):
    """keyword arguments of Context.adaptive_set_params for a world"""
    p = dict(min_samples=MIN_SAMPLES, step=STEP, dark=DARK, dilate=1, flags=0)
    p.update(kw)
    p.setdefault("threshold", world["threshold"][p["dilate"]])
    return p
