"""Numpy restatement of the rippled reads (include/datum_ocean_hip.h: "rippled reads"): the mesh, the surface query and the ray cast of the
summed surface with the ripple layer on top.  Built from blend64, ripple64, ray64 and gen64; nothing of them is copied.

Two forms:
  * float32, where the statement is bit for bit: the height addition (record32, vertex32's z) and the cast over a height callable
    (cast32: ray64.cast32 over the rippled records);
  * float64, for the normals and the mesh: blend64's float64 record and staged mesh DOWNSTREAM OF THE LAYER'S fp32 SAMPLE (ripple64.sample32,
    which the device's sampler is pinned against bit for bit), as gen64.staged64 is float64 downstream of gen64.ray32's fp32 values.  The
    layer enters blend64.slopes64 as one more sampled "normal" m = (-1/2 d eta/dx, -1/2 d eta/dy, 1): m.x / m.z is its slope term.

`mistake` plants the errors tests/test_rippled64.py names:
  "at_b"        the layer sampled at the solved base point's P(b) instead of the asked q
  "sign"        the slope's sign flipped
  "no_half"     the 1/2 left out
  "rate"        eta_t taken for eta
  "at_position" the mesh sampled at position.xy instead of position.xy - D.xy

The bars of the normals.  Two comparisons, two bars:
  * against the float64 form (record64, mesh64) the parent's bars hold the parent's own error -- K_NRM eps tex of tests/test_gpu_blend.py,
    dominated by the rounding of the texel coordinate -- and the layer's share is added on top as K_RIPN eps.  That bar is wide;
  * the TIGHT one needs no float64 map fetch.  Without swell the query's frame is constant (flat_normal64), so the summed slopes can be
    read back from the parent's own record: dn = (n.x, -n.y, n.z), p = dn.xy / dn.z.  relift64 forms the rippled normal from the parent's
    fp32 normal and the layer's fp32 sample in float64; normal32 is the fp32 restatement of what the kernel does behind the sums
    (rippled_slope, normalize3 twice through the constant frame, the reciprocal square root taken within one ulp either way).
    K_RIPN is three times the worst |normal32(p') - relift64(normal32(p), s)| / (eps (1 + |p'|^2)) over slopes and samples of the tests'
    range, measured by tests/test_rippled64.py::test_the_bar_of_the_normals on the CPU: worst 3.22, K_RIPN = 10 (the MI355X reaches 1.00).
"""

from types import SimpleNamespace

import numpy as np

import blend64
import ray64
import ripple64

F = np.float32
MISTAKES = ("at_b", "sign", "no_half", "rate", "at_position")
K_RIPN = 10.0                 # 3 x the CPU-measured 3.22 (test_the_bar_of_the_normals), rounded up; the MI355X measures 1.00


def lift32(height, samples, mistake=None):
    """the rippled height: one fp32 addition"""
    h, s = np.asarray(height, F), np.asarray(samples, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        out = h + s[:, 3 if mistake == "rate" else 0]
    assert out.dtype == F
    return out


def slope32(p, d, mistake=None):
    """p + (-0.5f * d): one fp32 product and one addition"""
    k = F(0.5) if mistake == "sign" else F(-1.0) if mistake == "no_half" else F(-0.5)
    with np.errstate(all="ignore"):
        out = np.asarray(p, F) + (k * np.asarray(d, F))
    assert out.dtype == F
    return out


def record32(recs, samples, mistake=None):
    """the fields of the rippled record that are stated bit for bit, from the parent's records [n, 8] and the layer's samples [n, 4] at the
    same points: field 2 lifted, fields 0, 1, 3 and 7 the parent's; fields 4-6 are left NaN (they are the float64 form's)"""
    r = np.array(recs, F).reshape(-1, 8)
    out = r.copy()
    out[:, 2] = lift32(r[:, 2], samples, mistake)
    out[:, 4:7] = np.nan
    out[np.isnan(r[:, 0])] = np.nan
    return out


def _layer_normal(samples, mistake):
    s = np.asarray(samples, np.float64).reshape(-1, 4)
    k = 0.5 if mistake == "sign" else -1.0 if mistake == "no_half" else -0.5
    return np.stack([k * s[:, 1], k * s[:, 2], np.ones(len(s))])


def record64(maps_list, foams, mode, scales, s, layer, points, iterations, mistake=None):
    """(M, 8) float64 rippled records: blend64's with the layer's sample (layer.sample: fp32, the bits) behind the list's slopes and on the
    height.  `layer`: a ripple64.Layer or anything with .sample(points)"""
    pts = np.asarray(points, F).reshape(-1, 2)
    where = pts
    if mistake == "at_b":
        # the solve's first iterate b_1 = q + (q - V(q).xy), from the record of zero iterations: a base point, off q by the displacement
        plain = blend64.surface_blend64(maps_list, foams, mode, scales, s, pts, 0)
        where = (2 * pts.astype(np.float64) - plain[:, :2]).astype(F)
    safe = np.where(np.isfinite(where).all(1)[:, None], where, F(0))
    smp = layer.sample(safe)
    inner = blend64.slopes64

    def with_layer(samples, m=None):
        return inner(list(samples) + [_layer_normal(smp, mistake)], m)

    blend64.slopes64 = with_layer
    try:
        out = blend64.surface_blend64(maps_list, foams, mode, scales, s, pts, iterations)
    finally:
        blend64.slopes64 = inner
    out[:, 2] = out[:, 2] + smp[:, 3 if mistake == "rate" else 0].astype(np.float64)
    return out


def _normalize32(x, y, z, ulp):
    """normalize3 of ocean_surface.hip in fp32: fma sums, a reciprocal square root off by `ulp` ulps, three products"""
    x, y, z = (np.asarray(v, F) for v in (x, y, z))
    ss = (z.astype(np.float64) * z + (y.astype(np.float64) * y + (x * x).astype(np.float64)).astype(F)).astype(F)
    inv = (1.0 / np.sqrt(ss.astype(np.float64))).astype(F)
    inv = (inv * F(1.0 + ulp * 2.0 ** -23)).astype(F)
    return x * inv, y * inv, z * inv


def normal32(px, py, ulp=0):
    """the record's normal of the summed slopes (px, py) without swell, in fp32 as blend_surface_normal forms it: dn = normalize(p, 1), the
    constant frame (x, -y, z) -- its products with 1 and 0 are exact -- and the second normalize"""
    nx, ny, nz = _normalize32(px, py, np.ones_like(np.asarray(px, F)), ulp)
    return np.stack(_normalize32(nx, -ny, nz, -ulp), 1)


def relift64(normal, samples):
    """the rippled normal without swell from the PARENT's normal [n, 3] (fp32 bits) and the layer's samples [n, 4], in float64: the summed
    slopes read back through the constant frame, the layer's share added, normalized; and |p'|^2 for the bar"""
    n, s = np.asarray(normal, np.float64), np.asarray(samples, np.float64).reshape(-1, 4)
    px, py = n[:, 0] / n[:, 2] - 0.5 * s[:, 1], -n[:, 1] / n[:, 2] - 0.5 * s[:, 2]
    v = np.stack([px, -py, np.ones_like(px)], 1)
    return v / np.sqrt((v * v).sum(1))[:, None], px * px + py * py


def flat_normal64(samples):
    """the rippled normal over a flat FFT surface without swell: dn = normalize(-1/2 d eta/dx, -1/2 d eta/dy, 1) through the query's frame,
    which without swell is t0 = (1, 0, 0), t2 = (0, 0, 1), t1 = t0 x t2 = (0, -1, 0): the record holds (dn.x, -dn.y, dn.z), as it does for
    every cascade's own slope (blend_surface_normal, gen.comp:101-120)"""
    n = _layer_normal(samples, None)
    return (n / np.sqrt((n * n).sum(0))).T * np.array([1.0, -1.0, 1.0])


def vertex32(verts, layer, mistake=None, position=None):
    """the rippled mesh's bit-for-bit part from gen_blend's vertices [sy, sx, 12]: x, y, u, v the parent's, z lifted by the layer's height
    at the stored (x, y); the normal and the tangent left NaN.  `position` [sy, sx, 2] is needed by the planted mistake alone"""
    v = np.array(verts, F)
    at = v[..., :2] if mistake != "at_position" else np.asarray(position, F)[..., :2]
    smp = layer.sample(at.reshape(-1, 2))
    out = v.copy()
    out[..., 2] = lift32(v[..., 2].reshape(-1), smp, mistake).reshape(v.shape[:2])
    out[..., 5:11] = np.nan
    return out


def mesh64(s, maps_list, scales, ray, layer, mistake=None):
    """blend64.staged_blend64 with the layer: sampled at the staged vertex's own (x, y) rounded to fp32 (the floats the vertex stores)"""
    plain = blend64.staged_blend64(s, maps_list, scales, ray)
    at = plain.vertices[..., :2] if mistake != "at_position" else plain.position[..., :2]
    smp = layer.sample(at.astype(F).reshape(-1, 2))
    shape = plain.vertices.shape[:2]
    inner = blend64.slopes64

    def with_layer(samples, m=None):
        return inner(list(samples) + [_layer_normal(smp, mistake).reshape((3,) + shape)], m)

    blend64.slopes64 = with_layer
    try:
        out = blend64.staged_blend64(s, maps_list, scales, ray)
    finally:
        blend64.slopes64 = inner
    out.vertices[..., 2] = out.vertices[..., 2] + smp[:, 3 if mistake == "rate" else 0].astype(np.float64).reshape(shape)
    return out


def cast32(record_fn, rays, S, R):
    """the rippled cast in float32: ray64.cast32, unchanged, over the rippled records (record_fn(points) -> [n, 8], field 2 the rippled
    height); .records is what datum_ocean_read_rays_rippled gives, bit for bit, where record_fn is datum_ocean_read_surface_blend_rippled"""
    return ray64.cast32(record_fn, rays, S, R)


def analytic32(height_fn, layer, mistake=None):
    """a record function for cast32 over an analytic fp32 height(x, y) plus the layer: what tests/cpu/rippled_emul.cpp walks"""
    def fn(q):
        q = np.asarray(q, F).reshape(-1, 2)
        rec = np.zeros((len(q), 8), F)
        fin = np.isfinite(q).all(1)
        safe = np.where(fin[:, None], q, F(0))
        rec[:, 2] = lift32(height_fn(safe[:, 0], safe[:, 1]), layer.sample(safe), mistake)
        rec[~fin] = np.nan
        return rec
    return fn


def bump(layer, I, J, height):
    """one raised cell (I, J) in a layer at rest"""
    eta = np.zeros((layer.R, layer.R), layer.T)
    eta[J - layer.oy, I - layer.ox] = height
    layer.set_window(eta, np.zeros_like(eta))
    return SimpleNamespace(x=(I + 0.5) * float(layer.s), y=(J + 0.5) * float(layer.s), height=height)
