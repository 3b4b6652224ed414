"""The shading schedule of the training renders and the light of each view.

Schedule and light distribution are the upstream trainers' (stable-dreamfusion's `train_step`, which the latent-NeRF
trainer this package mirrors follows): before `optim.start_shading_iter` every step renders the plain albedo; from that
step on a uniform u decides per step -- u > 0.8 albedo, 0.4 < u <= 0.8 textureless, otherwise lambertian, both with
ambient 0.1 -- and the light of a view sits at its camera position plus a standard normal deviate, normalised
(`safe_normalize(rays_o[0] + torch.randn(3))` upstream).

Every number here comes from the counter-based stream of (optim.seed, train_step[, view]) that also gives the poses
(distributed.pose_uniforms): a resumed run and every rank of a data-parallel run reproduce the draws without any state
or communication.  All views of one step share the shading kind."""
import math

from .distributed import pose_uniforms

AMBIENT = 0.1                      # ambient share of both shaded kinds (upstream: ambient_ratio = 0.1)
KINDS = ("albedo", "textureless", "lambertian")
# stream tags in pose_uniforms' view slot, far from any view index
_KIND_TAG = 0x5AD10000
_LIGHT_TAG = 0x11A70000


def shading_kind(seed, step, start_iter):
    """The shading of training step `step` (1-based, Trainer.train_step): 'albedo', 'textureless' or 'lambertian'."""
    if start_iter is None or int(step) < int(start_iter):
        return "albedo"
    u = pose_uniforms(seed, step, _KIND_TAG, 1)[0]
    if u > 0.8:
        return "albedo"
    if u > 0.4:
        return "textureless"
    return "lambertian"


def schedule(seed, first, last, start_iter):
    """[shading_kind(step) for step in first .. last]."""
    return [shading_kind(seed, s, start_iter) for s in range(int(first), int(last) + 1)]


def light_direction(seed, step, view, eye):
    """Unit vector toward the light of view `view` at step `step`: normalize(eye + N(0, I)), eye the camera position;
    the three deviates are Box-Muller transforms of four uniforms of the (seed, step, view) stream.  Plain doubles."""
    u = pose_uniforms(seed, step, _LIGHT_TAG + int(view), 4)
    r0 = math.sqrt(-2.0 * math.log(1.0 - u[0]))          # (1 - u in (0, 1]: the logarithm is finite)
    r1 = math.sqrt(-2.0 * math.log(1.0 - u[2]))
    z = (r0 * math.cos(2.0 * math.pi * u[1]), r0 * math.sin(2.0 * math.pi * u[1]), r1 * math.cos(2.0 * math.pi * u[3]))
    v = [float(e) + d for e, d in zip(eye, z)]
    n = max(math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), 1e-20)
    return (v[0] / n, v[1] / n, v[2] / n)


def shade_row(seed, step, view, eye, kind):
    """The five floats of a view's shade record (raymarching.shade_fd): (l_x, l_y, l_z, ambient, textureless)."""
    l = light_direction(seed, step, view, eye)
    return (l[0], l[1], l[2], AMBIENT, 1.0 if kind == "textureless" else 0.0)
