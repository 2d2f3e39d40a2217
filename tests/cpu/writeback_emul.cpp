// The host's bookkeeping of the lazy phase write-back (datum_amd/csrc/ocean_writeback.h) behind a C interface, for tests/test_phase_writeback_model.py:
// the very struct the HIP module keeps in its handle, no HIP call in sight.

#include "../../datum_amd/csrc/ocean_writeback.h"

using ocean::PhaseWriteback;

namespace
{
  int give(PhaseWriteback::Launch const &l, float *dt, int *store)
  {
    for(int i = 0; i < l.ndt; ++i)
      dt[i] = l.dt[i];

    *store = l.store ? 1 : 0;

    return l.ndt;
  }
}

extern "C"
{
  int writeback_max_pending() { return ocean::MAX_PENDING; }

  void *writeback_new() { return new PhaseWriteback; }
  void writeback_delete(void *w) { delete static_cast<PhaseWriteback*>(w); }

  int writeback_fits(void *w, int n) { return static_cast<PhaseWriteback*>(w)->fits(n) ? 1 : 0; }
  void writeback_clear(void *w) { static_cast<PhaseWriteback*>(w)->clear(); }

  // the launch's dt's into dt[MAX_PENDING], its store flag into *store; returns ndt
  int writeback_step(void *w, float const *pending, int n, int every, float *dt, int *store)
  {
    return give(static_cast<PhaseWriteback*>(w)->step(pending, n, every), dt, store);
  }

  int writeback_repeat(void *w, float *dt, int *store)
  {
    return give(static_cast<PhaseWriteback*>(w)->repeat(), dt, store);
  }
}
