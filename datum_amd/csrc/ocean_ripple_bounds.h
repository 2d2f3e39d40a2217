// ocean_ripple_bounds.h -- bounds of the ripple layer (include/datum_ocean_hip.h: datum_ocean_reduce_ripple_bounds) stated once: the record,
// the fold of a cell into it and of two partial records into one, and the slab a blend list's records and the layer's record give under a
// set -- the slab of the rippled water, for datum_ocean_surface_slab_rippled and for the bounded rippled cast, which is ocean_bounds.h's
// ray_search_bounded over ocean_rippled.h's height with this slab.
//
// Host/device neutral so that a CPU can walk it (tests/cpu/ripple_bounds_emul.cpp, tests/test_ripple_bounds_emul.py): the kernels of
// ocean_ripple_bounds.hip and datum_ocean_surface_slab_rippled call these functions, there is no second copy.  Built with
// -ffp-contract=off wherever it is built: every product and sum is one fp32 operation, rounded as written; there is no fused
// multiply-add here.

#pragma once

#include <math.h>

#include "ocean_bounds.h"
#include "ocean_rippled.h"

namespace ocean
{
  constexpr int RIPPLE_BOUNDS_FIELDS = DATUM_OCEAN_RIPPLE_BOUNDS_RECORD_FLOATS;

  static_assert(RIPPLE_BOUNDS_FIELDS == 8, "a record is two 16-byte stores");

  // the extrema of eta and of the rate over the cells of the layer's current state, the cells with a non-finite eta or rate, and the cells
  // that are not at rest.  A NaN enters no extremum (fminf, fmaxf), an infinity does; either is counted, in both counts
  struct RippleBounds
  {
    float etamin, etamax, ratemin, ratemax;
    unsigned int nonfinite, active;
  };

  OR_HD RippleBounds ripple_bounds_identity()
  {
    RippleBounds b;
    b.etamin = b.ratemin = INFINITY;
    b.etamax = b.ratemax = -INFINITY;
    b.nonfinite = b.active = 0;
    return b;
  }

  OR_HD void ripple_bounds_cell(RippleBounds &b, float eta, float rate)
  {
    b.etamin = fminf(b.etamin, eta); b.etamax = fmaxf(b.etamax, eta);
    b.ratemin = fminf(b.ratemin, rate); b.ratemax = fmaxf(b.ratemax, rate);

    b.nonfinite += (ray_finite(eta) && ray_finite(rate)) ? 0u : 1u;
    b.active += (eta != 0.0f || rate != 0.0f) ? 1u : 0u;          // (a NaN differs from 0)
  }

  // order-independent but for the sign of a zero extremum
  OR_HD void ripple_bounds_merge(RippleBounds &b, RippleBounds const &o)
  {
    b.etamin = fminf(b.etamin, o.etamin); b.etamax = fmaxf(b.etamax, o.etamax);
    b.ratemin = fminf(b.ratemin, o.ratemin); b.ratemax = fmaxf(b.ratemax, o.ratemax);

    b.nonfinite += o.nonfinite;
    b.active += o.active;
  }

  // the record: etamin, etamax, ratemin, ratemax, nonfinite, active (R * R <= 2^20 cells: exact), 0, 0
  OR_HD void ripple_bounds_record(RippleBounds const &b, float *rec)
  {
    rec[0] = b.etamin; rec[1] = b.etamax;
    rec[2] = b.ratemin; rec[3] = b.ratemax;
    rec[4] = (float)b.nonfinite;
    rec[5] = (float)b.active;
    rec[6] = 0.0f;
    rec[7] = 0.0f;
  }

  // The slab of the rippled water: bounds_slab's sums over the list, then the layer as one more entry behind it.  The layer displaces
  // nothing horizontally (reach is bounds_slab's), and a point outside the window reads 0, so 0 always lies inside the layer's interval:
  // elo = fminf(etamin, 0), ehi = fmaxf(etamax, 0).  Between zlo and zhi lies every height the rippled query can give for the list, the set
  // and the layer: the parent's height inside the parent's un-padded sums up to the parent's stated roundings, the bilinear eta beyond its
  // four cells' extrema by at most a few ulp of max |eta|, one more rounded addition; pad, 2^-16 of the magnitudes with the layer's among
  // them, covers these.  A listed cascade or the layer with a non-finite value: zlo = zhi = NaN, which decides no sample.
  // (bounds_slab keeps its text: its sums are formed again here, line for line, because the pad comes behind the layer's terms)
  // layer: the layer's record, [RIPPLE_BOUNDS_FIELDS]; the other arguments are bounds_slab's
  OR_HD BoundsSlab ripple_bounds_slab(float const *records, int const *cascades, int count, float basez, float A, float gx, float gy, float const *layer)
  {
    float const absa = fabsf(A);

    float mag = fabsf(basez) + absa;
    float hi = basez + absa;
    float lo = basez - absa;
    float rx = fabsf(gx), ry = fabsf(gy);
    bool nonfinite = false;

    for(int c = 0; c < count; ++c)
    {
      float const *r = records + (size_t)cascades[c] * BOUNDS_FIELDS;

      mag = mag + fmaxf(fabsf(r[0]), fabsf(r[1]));
      hi = hi + r[1];
      lo = lo + r[0];
      rx = rx + fmaxf(fabsf(r[2]), fabsf(r[3]));
      ry = ry + fmaxf(fabsf(r[4]), fabsf(r[5]));

      nonfinite = nonfinite || r[6] > 0.0f;
    }

    float const elo = fminf(layer[0], 0.0f);
    float const ehi = fmaxf(layer[1], 0.0f);

    mag = mag + fmaxf(fabsf(elo), fabsf(ehi));
    hi = hi + ehi;
    lo = lo + elo;

    nonfinite = nonfinite || layer[4] > 0.0f;

    float const pad = mag * 1.52587890625e-05f;         // 2^-16

    BoundsSlab s;
    s.zhi = nonfinite ? __builtin_nanf("") : hi + pad;
    s.zlo = nonfinite ? __builtin_nanf("") : lo - pad;
    s.reachx = rx;
    s.reachy = ry;
    return s;
  }
}
