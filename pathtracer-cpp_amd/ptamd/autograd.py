"""trace() along fixed rays as a differentiable function of the scene's colours and emissions.

`trace_radiance(renderer, origins, directions, color, emit, depth, samples, seed)` returns the
radiance `Renderer.trace` would give on a scene whose triangles carry `color` / `emit`, and its
backward pass returns the exact gradients with respect to both (Renderer.trace_grad: the paths do
not depend on either, so the radiance is a polynomial in them). With `light_sampling` the value is
`Renderer.trace_nee`'s (the same expectation, a smaller variance) and the backward pass
Renderer.trace_nee_grad's, exact in the same way. `render_radiance(renderer, camera, color, emit,
depth, samples, seed)` is the same for the rendered image along its own camera rays
(Renderer.render_grad). torch is imported on first use.
"""
from __future__ import annotations

_fn = None


def _function():
    global _fn
    if _fn is not None:
        return _fn
    import torch

    class TraceRadiance(torch.autograd.Function):
        @staticmethod
        def forward(ctx, renderer, origins, directions, color, emit, depth, samples, seed, states, light_sampling, mis):
            c = None if color is None else color.detach().to(torch.float32).contiguous()
            e = None if emit is None else emit.detach().to(torch.float32).contiguous()
            ctx.call = _grad_call(renderer, light_sampling, mis)
            res, _ = ctx.call(origins, directions, None, depth, samples=samples, seed=seed, states=states,
                              color=c, emit=e, want=("rgb",))
            ctx.renderer, ctx.rays, ctx.mats = renderer, (origins, directions, states), (c, e)
            ctx.args = (depth, samples, seed)
            ctx.dtypes = (None if color is None else color.dtype, None if emit is None else emit.dtype)
            return res["rgb"]

        @staticmethod
        def backward(ctx, grad_rgb):
            origins, directions, states = ctx.rays
            c, e = ctx.mats
            depth, samples, seed = ctx.args
            need_c = c is not None and ctx.needs_input_grad[3]
            need_e = e is not None and ctx.needs_input_grad[4]
            want = tuple(k for k, need in (("color", need_c), ("emit", need_e)) if need)
            g_c = g_e = None
            if want:
                g = grad_rgb.detach().to(torch.float32).contiguous()
                res, _ = ctx.call(origins, directions, g, depth, samples=samples, seed=seed, states=states,
                                  color=c, emit=e, want=want)
                if need_c:
                    g_c = res["color"].to(ctx.dtypes[0])
                if need_e:
                    g_e = res["emit"].to(ctx.dtypes[1])
            return None, None, None, g_c, g_e, None, None, None, None, None, None

    _fn = TraceRadiance
    return _fn


_render_fn = None


def _render_function():
    global _render_fn
    if _render_fn is not None:
        return _render_fn
    import torch

    class RenderRadiance(torch.autograd.Function):
        @staticmethod
        def forward(ctx, renderer, camera, color, emit, depth, samples, seed, light_sampling, mis):
            c = None if color is None else color.detach().to(torch.float32).contiguous()
            e = None if emit is None else emit.detach().to(torch.float32).contiguous()
            if mis and not light_sampling:
                raise ValueError("mis needs light_sampling")
            ctx.kw = dict(samples=samples, depth=depth, seed=seed, light_sampling=light_sampling, mis=mis)
            res, _ = renderer.render_grad(camera, None, color=c, emit=e, want=("rgb",), **ctx.kw)
            ctx.renderer, ctx.camera, ctx.mats = renderer, camera, (c, e)
            ctx.dtypes = (None if color is None else color.dtype, None if emit is None else emit.dtype)
            rgb = res["rgb"]
            if not torch.is_tensor(rgb):  # neither material given: the numpy path answered
                rgb = torch.from_numpy(rgb).to(torch.device("cuda", renderer.device))
            return rgb

        @staticmethod
        def backward(ctx, grad_img):
            c, e = ctx.mats
            need_c = c is not None and ctx.needs_input_grad[2]
            need_e = e is not None and ctx.needs_input_grad[3]
            want = tuple(k for k, need in (("color", need_c), ("emit", need_e)) if need)
            g_c = g_e = None
            if want:  # one gradient-only call: no radiance is written
                g = grad_img.detach().to(torch.float32).contiguous()
                res, _ = ctx.renderer.render_grad(ctx.camera, g, color=c, emit=e, want=want, **ctx.kw)
                if need_c:
                    g_c = res["color"].to(ctx.dtypes[0])
                if need_e:
                    g_e = res["emit"].to(ctx.dtypes[1])
            return None, None, g_c, g_e, None, None, None, None, None

    _render_fn = RenderRadiance
    return _render_fn


def _grad_call(renderer, light_sampling: bool, mis: bool):
    """Renderer.trace_grad, or with `light_sampling` Renderer.trace_nee_grad bound to `mis`."""
    if not light_sampling:
        if mis:
            raise ValueError("mis needs light_sampling")
        return renderer.trace_grad
    return lambda *args, **kw: renderer.trace_nee_grad(*args, mis=mis, **kw)


def render_radiance(renderer, camera, color, emit, depth, samples=1, seed=1, light_sampling=False, mis=False):
    """image (H, W, 3) float32 on the renderer's device: Renderer.render's image (with
    `light_sampling` Renderer.render_nee's, `mis` its weighted form) for `camera` at the given
    `color` and `emit` ((num_tris, 3) tensors on that device, either may be None = the scene's),
    differentiable with respect to both. Every sample of a pixel runs along its own jittered camera
    ray; the backward pass is one gradient-only Renderer.render_grad call. The light table stays the
    scene's whatever `emit` holds."""
    return _render_function().apply(renderer, camera, color, emit, depth, samples, seed, bool(light_sampling), bool(mis))


def trace_radiance(renderer, origins, directions, color, emit, depth, samples=1, seed=1, states=None,
                   light_sampling=False, mis=False):
    """rgb (n, 3) float32 on the rays' device: trace() along the rays at the given `color` and
    `emit` ((num_tris, 3) tensors on the renderer's device, either may be None = the scene's),
    differentiable with respect to both. origins, directions (and states) are contiguous float32
    (32-bit integer) tensors on that device, as for Renderer.trace_grad. `light_sampling`: the
    light-sampling estimator (Renderer.trace_nee's value, Renderer.trace_nee_grad's gradients),
    with `mis` its weighted form; the light table stays the scene's whatever `emit` holds."""
    return _function().apply(renderer, origins, directions, color, emit, depth, samples, seed, states,
                             bool(light_sampling), bool(mis))
