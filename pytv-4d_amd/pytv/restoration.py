"""2-D / 3-D ``denoise_tv_chambolle`` front-end with scikit-image's calling convention, on top of the device
resident Chambolle-Pock solver (README.md:260 of the reference lists this as a to-do).

scikit-image minimises  sum |grad u| + (1 / (2 weight)) |u - f|^2  with forward differences, i.e.
1/2 |u - f|^2 + weight * TV_upwind(u): the same objective as ``solvers.ChambollePock(f, weight, scheme="upwind")``.
Its iteration (Chambolle 2004) differs from Chambolle-Pock 2011, so iterates differ; the minimiser is the same.
"""
import math

import torch

from . import _native as _nv
from .solvers import (AcceleratedChambollePock, AdaptiveHuberChambollePock, AdaptiveTVChambollePock, ChambollePock, HuberChambollePock, PoissonChambollePock,
                      RobustChambollePock, VectorialTVChambollePock, WeightedChambollePock)
from .tv_operators_GPU import _to_device

__all__ = ["denoise_tv_chambolle", "denoise_tv_robust", "denoise_tv_poisson", "denoise_tv_huber", "denoise_tv_weighted", "denoise_tv_adaptive",
           "denoise_tv_adaptive_huber", "edge_stopping_weights", "denoise_tv_vectorial"]


def denoise_tv_chambolle(image, weight=0.1, eps=2.0e-4, max_num_iter=200, *, scheme="upwind", check_every=10, rel_gap=None,
                         accelerated=False):
    """Total-variation denoising of a 2-D (rows, cols) or 3-D (planes, rows, cols) image.

    weight : denoising weight (larger = smoother), as in scikit-image.
    eps    : stop when the relative change of the objective over ``check_every`` iterations drops below eps.
    rel_gap: None (the default) = the rule above; a number = stop when the duality gap certifies the answer instead,
             gap <= rel_gap * objective at a check (``ChambollePock.run_until``: 1/2 |u - u*|^2 <= gap); ``eps`` is then ignored.
    accelerated: False (the default) = ``solvers.ChambollePock``; True = ``solvers.AcceleratedChambollePock`` (O(1/k^2): about a third of
             the iterations to a given ``rel_gap`` for the one-sided schemes).  Its loss history is a progress indicator (the TV of the
             extrapolated point), which is what the ``eps`` rule then watches; prefer ``rel_gap`` with it.
    Returns an array of the input's kind (numpy in -> numpy out, torch in -> device tensor), floating point."""
    was_torch = isinstance(image, torch.Tensor)
    x, _ = _to_device(image)
    if x.dim() == 2:
        vol = x.reshape(1, 1, *x.shape)
    elif x.dim() == 3:
        vol = x.reshape(x.shape[0], 1, x.shape[1], x.shape[2])
    else:
        raise ValueError("denoise_tv_chambolle: 2-D or 3-D images only (use pytv.solvers for 4-D data)")
    if accelerated:
        cp = AcceleratedChambollePock(vol.contiguous(), float(weight), scheme=scheme, reg_z_over_reg=1.0)
    else:
        cp = ChambollePock(vol.contiguous(), float(weight), scheme=scheme, reg_z_over_reg=1.0)
    prev, done = None, 0
    if rel_gap is not None:
        cp.run_until(rel_gap, max_num_iter, check_every)
        done = max_num_iter
    while done < max_num_iter:
        n = min(check_every, max_num_iter - done)
        loss = cp.run(n)
        done += n
        e = float(loss[-1])
        if prev is not None and abs(prev - e) <= eps * max(abs(prev), 1e-30):
            break
        prev = e
    out = cp.result().reshape(x.shape)
    return out if was_torch else out.detach().cpu().numpy()


def denoise_tv_robust(image, weight=1.0, fidelity="l1", delta=None, rel_res=1e-2, max_num_iter=400, *, scheme="upwind", tau=None,
                      check_every=10):
    """Total-variation denoising of a 2-D (rows, cols) or 3-D (planes, rows, cols) image with a ROBUST data term -- impulse noise (dead or
    hot pixels, zingers, salt and pepper), where the quadratic term of ``denoise_tv_chambolle`` fails: minimises F(u - f) + weight * TV(u).

    weight  : denoising weight (larger = smoother).  For "l1" it is in units of one: a structure survives roughly when its area / perimeter
              ratio exceeds ``weight``; it does not scale with the grey levels.
    fidelity: "l1" (|u - f|_1), "huber" (quadratic below ``delta`` grey levels, linear beyond; ``delta`` required) or "l2".
    rel_res : stop when the optimality residual has dropped to rel_res times that of the start (``RobustChambollePock.run_until``), checked
              every ``check_every`` iterations, or after ``max_num_iter`` iterations.
    tau     : the primal step in grey levels.  None = the balanced default, which is slow for "l1" / "huber" on data with a wide range: a few
              grey levels (tau = 5 on 0..255 data) converges far faster (``RobustChambollePock``).
    Returns an array of the input's kind (numpy in -> numpy out, torch in -> device tensor), floating point."""
    was_torch = isinstance(image, torch.Tensor)
    x, _ = _to_device(image)
    if x.dim() == 2:
        vol = x.reshape(1, 1, *x.shape)
    elif x.dim() == 3:
        vol = x.reshape(x.shape[0], 1, x.shape[1], x.shape[2])
    else:
        raise ValueError("denoise_tv_robust: 2-D or 3-D images only (use pytv.solvers for 4-D data)")
    cp = RobustChambollePock(vol.contiguous(), float(weight), fidelity=fidelity, delta=delta, scheme=scheme, reg_z_over_reg=1.0, tau=tau)
    cp.run_until(rel_res, max_num_iter, check_every)
    out = cp.result().reshape(x.shape)
    return out if was_torch else out.detach().cpu().numpy()


def denoise_tv_poisson(image, weight=1.0, rel_res=1e-2, max_num_iter=400, *, scheme="upwind", tau=None, check_every=10):
    """Total-variation denoising of a 2-D (rows, cols) or 3-D (planes, rows, cols) image of photon COUNTS (Poisson noise: the variance of a
    pixel equals its mean, so dark regions are cleaner than bright ones and a quadratic data term weighs them wrongly): minimises
    KL(f, u) + weight * TV(u) over u >= 0 with the generalised Kullback-Leibler divergence KL(f, u) = sum (u - f + f log(f / u)).

    image   : the counts, finite and >= 0 (ValueError otherwise); not rescaled -- the model depends on the absolute count level.
    weight  : denoising weight (larger = smoother).
    rel_res : stop when the optimality residual has dropped to rel_res times that of the start (``PoissonChambollePock.run_until``), checked
              every ``check_every`` iterations, or after ``max_num_iter`` iterations.
    tau     : the primal step; None = the balanced default of ``PoissonChambollePock``.
    Returns an array of the input's kind (numpy in -> numpy out, torch in -> device tensor), floating point, >= 0."""
    was_torch = isinstance(image, torch.Tensor)
    x, _ = _to_device(image)
    if x.dim() == 2:
        vol = x.reshape(1, 1, *x.shape)
    elif x.dim() == 3:
        vol = x.reshape(x.shape[0], 1, x.shape[1], x.shape[2])
    else:
        raise ValueError("denoise_tv_poisson: 2-D or 3-D images only (use pytv.solvers for 4-D data)")
    cp = PoissonChambollePock(vol.contiguous(), float(weight), scheme=scheme, reg_z_over_reg=1.0, tau=tau)
    cp.run_until(rel_res, max_num_iter, check_every)
    out = cp.result().reshape(x.shape)
    return out if was_torch else out.detach().cpu().numpy()


def denoise_tv_weighted(image, weights, weight=0.1, lower=None, upper=None, rel_res=1e-2, max_num_iter=400, *, scheme="upwind", tau=None,
                        check_every=10):
    """Total-variation denoising / INPAINTING of a 2-D (rows, cols) or 3-D (planes, rows, cols) image with a per-pixel data weight and
    optional bounds: minimises 1/2 sum weights (u - f)^2 + weight * TV(u) over lower <= u <= upper.

    weights : an array of the image's shape.  bool: True = the pixel is known, False = unknown (a dead detector pixel, a masked region: TV
              fills it in, whatever value the image holds there); floating point: finite and >= 0, e.g. 1 / variance per pixel.
    weight  : denoising weight (larger = smoother), as in ``denoise_tv_chambolle`` (which is ``weights`` = 1 everywhere, no bounds).
    lower, upper : bounds on the result that hold exactly (non-negativity, a normalised range); None = none on that side.
    rel_res : stop when the optimality residual has dropped to rel_res times that of the start (``WeightedChambollePock.run_until``),
              checked every ``check_every`` iterations, or after ``max_num_iter`` iterations.
    tau     : the primal step; None = the balanced default of ``WeightedChambollePock``.
    Returns an array of the input's kind (numpy in -> numpy out, torch in -> device tensor), floating point."""
    was_torch = isinstance(image, torch.Tensor)
    x, _ = _to_device(image)
    if x.dim() == 2:
        vol = x.reshape(1, 1, *x.shape)
    elif x.dim() == 3:
        vol = x.reshape(x.shape[0], 1, x.shape[1], x.shape[2])
    else:
        raise ValueError("denoise_tv_weighted: 2-D or 3-D images only (use pytv.solvers for 4-D data)")
    w = torch.as_tensor(weights, device=x.device)
    if tuple(w.shape) != tuple(x.shape):
        raise ValueError("denoise_tv_weighted: weights must have the shape of the image, %r (got %r)" % (tuple(x.shape), tuple(w.shape)))
    cp = WeightedChambollePock(vol.contiguous(), float(weight), w.reshape(vol.shape), lower=lower, upper=upper, scheme=scheme,
                               reg_z_over_reg=1.0, tau=tau)
    cp.run_until(rel_res, max_num_iter, check_every)
    out = cp.result().reshape(x.shape)
    return out if was_torch else out.detach().cpu().numpy()


def denoise_tv_huber(image, weight=0.1, alpha=1.0, rel_gap=1e-4, max_num_iter=200, *, scheme="upwind", check_every=10):
    """Denoising of a 2-D (rows, cols) or 3-D (planes, rows, cols) image with the HUBER-TV regulariser, the standard remedy for the
    staircasing of plain TV (smooth ramps coming back as terraces): minimises 1/2 |u - f|^2 + weight * sum h_alpha(|grad u|), where
    h_alpha is quadratic below a gradient magnitude ``alpha`` and linear -- TV -- above it (Chambolle & Pock 2011, section 6.2.1).

    weight : denoising weight (larger = smoother), as in ``denoise_tv_chambolle``.
    alpha  : the gradient magnitude, in grey levels per pixel, below which the model smooths instead of preserving an edge; finite and > 0
             (alpha -> 0 is ``denoise_tv_chambolle``).  It scales with the grey levels of the image.
    rel_gap: stop when the duality gap certifies the answer, gap <= rel_gap * objective at a check (``HuberChambollePock.run_until``:
             1/2 |u - u*|^2 <= gap), checked every ``check_every`` iterations, or after ``max_num_iter`` iterations.
    Returns an array of the input's kind (numpy in -> numpy out, torch in -> device tensor), floating point."""
    was_torch = isinstance(image, torch.Tensor)
    x, _ = _to_device(image)
    if x.dim() == 2:
        vol = x.reshape(1, 1, *x.shape)
    elif x.dim() == 3:
        vol = x.reshape(x.shape[0], 1, x.shape[1], x.shape[2])
    else:
        raise ValueError("denoise_tv_huber: 2-D or 3-D images only (use pytv.solvers for 4-D data)")
    cp = HuberChambollePock(vol.contiguous(), float(weight), float(alpha), scheme=scheme, reg_z_over_reg=1.0)
    cp.run_until(rel_gap, max_num_iter, check_every)
    out = cp.result().reshape(x.shape)
    return out if was_torch else out.detach().cpu().numpy()


def _as_volume(x, who):
    """a 2-D (rows, cols) or 3-D (planes, rows, cols) device tensor as the (Nz, 1, Ny, Nx) volume the solvers take"""
    if x.dim() == 2:
        return x.reshape(1, 1, *x.shape).contiguous()
    if x.dim() == 3:
        return x.reshape(x.shape[0], 1, x.shape[1], x.shape[2]).contiguous()
    raise ValueError("%s: 2-D or 3-D images only (use pytv.solvers for 4-D data)" % who)


def edge_stopping_weights(image, kappa, *, scheme="upwind"):
    """The edge-stopping weights g = 1 / (1 + (|grad image|_2 / kappa)^2) of a 2-D (rows, cols) or 3-D (planes, rows, cols) image: 1 where
    the image is flat, small across an edge whose gradient magnitude exceeds ``kappa`` -- the weighted TV of the segmentation and
    edge-preserving denoising literature, ``reg_weights`` of ``denoise_tv_adaptive`` / ``AdaptiveTVChambollePock``.

    kappa  : the gradient magnitude, in grey levels per pixel, at which the weight is 1/2; finite and > 0 (ValueError otherwise).
    scheme : the difference scheme of the gradient, that of the denoising call the weights are meant for.
    |grad image|_2 is the per-pixel norm over the channels of D image (tv_D + tv_l21, the differences the solver takes); the weights lie
    in (0, 1].  Returns an array of the input's kind and shape (numpy in -> numpy out, torch in -> device tensor), floating point."""
    kappa = float(kappa)
    if not (math.isfinite(kappa) and kappa > 0.0):
        raise ValueError("edge_stopping_weights: kappa must be finite and > 0")
    was_torch = isinstance(image, torch.Tensor)
    x, _ = _to_device(image)
    vol = _as_volume(x, "edge_stopping_weights")
    geo = _nv.Geometry(tuple(vol.shape), scheme, vol.dtype, vol.device, 1.0, 0.0, False, 0)
    d = torch.empty(geo.grad_shape, dtype=vol.dtype, device=vol.device)
    norms = torch.empty_like(vol)
    st = _nv.current_stream(vol.device)
    _nv.check(_nv.lib().tv_D(geo.ref, _nv.ptr(vol), None, None, _nv.ptr(d), st))
    _nv.check(_nv.lib().tv_l21(geo.ref, _nv.ptr(d), geo.nd, _nv.ptr(norms), _nv.ptr(geo.scalar()), _nv.ptr(geo.workspace()), st))
    norms.div_(kappa)
    g = torch.reciprocal(norms.mul_(norms).add_(1.0)).reshape(x.shape)
    return g if was_torch else g.detach().cpu().numpy()


def denoise_tv_adaptive(image, weight=0.1, reg_weights=None, rel_gap=1e-4, max_num_iter=200, *, scheme="upwind", check_every=10):
    """SPATIALLY ADAPTIVE total-variation denoising of a 2-D (rows, cols) or 3-D (planes, rows, cols) image: minimises
    1/2 |u - f|^2 + weight * sum_i reg_weights_i |grad u|_i -- the strength of the TV term varies from pixel to pixel.

    weight      : denoising weight (larger = smoother), as in ``denoise_tv_chambolle``.
    reg_weights : an array of the image's shape, finite and >= 0; None = all ones (``denoise_tv_chambolle``'s model).  Larger where the
                  noise is stronger; ``edge_stopping_weights(image, kappa)`` to smooth less across edges; 0 inside a region that must be
                  left as it is.
    rel_gap     : stop when the duality gap certifies the answer, gap <= rel_gap * objective at a check
                  (``AdaptiveTVChambollePock.run_until``: 1/2 |u - u*|^2 <= gap), checked every ``check_every`` iterations, or after
                  ``max_num_iter`` iterations.
    Returns an array of the input's kind (numpy in -> numpy out, torch in -> device tensor), floating point."""
    was_torch = isinstance(image, torch.Tensor)
    x, _ = _to_device(image)
    vol = _as_volume(x, "denoise_tv_adaptive")
    if reg_weights is None:
        g = torch.ones_like(vol)
    else:
        g = torch.as_tensor(reg_weights, device=x.device)
        if tuple(g.shape) != tuple(x.shape):
            raise ValueError("denoise_tv_adaptive: reg_weights must have the shape of the image, %r (got %r)" % (tuple(x.shape), tuple(g.shape)))
        g = g.reshape(vol.shape)
    cp = AdaptiveTVChambollePock(vol, float(weight), g, scheme=scheme, reg_z_over_reg=1.0)
    cp.run_until(rel_gap, max_num_iter, check_every)
    out = cp.result().reshape(x.shape)
    return out if was_torch else out.detach().cpu().numpy()


def denoise_tv_adaptive_huber(image, weight=0.1, reg_weights=None, alpha=1.0, rel_gap=1e-4, max_num_iter=200, *, scheme="upwind", check_every=10):
    """SPATIALLY ADAPTIVE HUBER-TV denoising of a 2-D (rows, cols) or 3-D (planes, rows, cols) image: minimises
    1/2 |u - f|^2 + weight * sum_i reg_weights_i h_alpha(|grad u|_i) -- ``denoise_tv_adaptive`` with the Huber function of
    ``denoise_tv_huber`` in place of the norm, so that the strongly smoothed flat and gently ramped regions do not come back as terraces.

    weight      : denoising weight (larger = smoother), as in ``denoise_tv_chambolle``.
    reg_weights : an array of the image's shape, finite and >= 0; None = all ones (``denoise_tv_huber``'s model).  Larger where the
                  noise is stronger; ``edge_stopping_weights(image, kappa)`` to smooth less across edges; 0 inside a region that must be
                  left as it is.
    alpha       : the gradient magnitude, in grey levels per pixel, below which the model smooths quadratically; finite and > 0.
    rel_gap     : stop when the duality gap certifies the answer, gap <= rel_gap * objective at a check
                  (``AdaptiveHuberChambollePock.run_until``: 1/2 |u - u*|^2 <= gap), checked every ``check_every`` iterations, or after
                  ``max_num_iter`` iterations.
    The iterations take the solver's default path (``AdaptiveHuberChambollePock``: the kernel pair, or one sweep on large volumes in the
    schemes where that measured faster).
    Returns an array of the input's kind (numpy in -> numpy out, torch in -> device tensor), floating point."""
    was_torch = isinstance(image, torch.Tensor)
    x, _ = _to_device(image)
    vol = _as_volume(x, "denoise_tv_adaptive_huber")
    if reg_weights is None:
        g = torch.ones_like(vol)
    else:
        g = torch.as_tensor(reg_weights, device=x.device)
        if tuple(g.shape) != tuple(x.shape):
            raise ValueError("denoise_tv_adaptive_huber: reg_weights must have the shape of the image, %r (got %r)"
                             % (tuple(x.shape), tuple(g.shape)))
        g = g.reshape(vol.shape)
    cp = AdaptiveHuberChambollePock(vol, float(weight), g, float(alpha), scheme=scheme, reg_z_over_reg=1.0)
    cp.run_until(rel_gap, max_num_iter, check_every)
    out = cp.result().reshape(x.shape)
    return out if was_torch else out.detach().cpu().numpy()


def denoise_tv_vectorial(image, weight=0.1, channel_axis=0, rel_gap=1e-4, max_num_iter=200, *, scheme="upwind", check_every=10):
    """CHANNEL-COUPLED (vectorial / joint) total-variation denoising of a multi-channel image: minimises
    1/2 |u - f|^2 + weight * sum_pixels ( sum_channels |grad u_c|^2 )^(1/2) -- one norm per pixel over ALL channels, so the channels keep
    their edges in the same places (colour images, dual- and multi-energy or multi-contrast stacks).

    image        : 3-D, channels along ``channel_axis`` and (rows, cols) in the remaining order -- (C, H, W) for ``channel_axis`` 0,
                   (H, W, C) for -1 --, or 4-D with planes as well: (Nz, C, H, W) after moving ``channel_axis`` to position 1.
                   ValueError for any other rank.
    weight       : denoising weight (larger = smoother), as in ``denoise_tv_chambolle``.  One channel is ``denoise_tv_chambolle``'s model.
    channel_axis : the axis of ``image`` that holds the channels (0 for 3-D input means (C, H, W); for 4-D input the planes are the first
                   of the remaining axes).
    rel_gap      : stop when the duality gap certifies the answer, gap <= rel_gap * objective at a check
                   (``VectorialTVChambollePock.run_until``: 1/2 |u - u*|^2 <= gap), checked every ``check_every`` iterations, or after
                   ``max_num_iter`` iterations.
    Returns an array of the input's kind (numpy in -> numpy out, torch in -> device tensor), floating point, with the input's shape and
    axis order."""
    was_torch = isinstance(image, torch.Tensor)
    x, _ = _to_device(image)
    if x.dim() not in (3, 4):
        raise ValueError("denoise_tv_vectorial: 3-D (channels, rows, cols) or 4-D (planes, channels, rows, cols) images only, "
                         "with the channels along channel_axis")
    moved = torch.movedim(x, channel_axis, 0 if x.dim() == 3 else 1)
    vol = (moved.unsqueeze(0) if x.dim() == 3 else moved).contiguous()
    cp = VectorialTVChambollePock(vol, float(weight), scheme=scheme, reg_z_over_reg=1.0)
    cp.run_until(rel_gap, max_num_iter, check_every)
    out = cp.result().reshape(moved.shape)
    out = torch.movedim(out, 0 if x.dim() == 3 else 1, channel_axis).contiguous()
    return out if was_torch else out.detach().cpu().numpy()
