// ocean_writeback.h -- the host's bookkeeping of the lazy phase write-back (plain C++: ocean_capi.hip uses it, tests/cpu/writeback_emul.cpp
// walks it on the CPU).
//
// The fused row pass applies a list of up to MAX_PENDING update_ocean dt's, in order, to the phase it loads.  It need not store the result:
// a later row pass that is handed the same dt's again, in front of the newer ones, arrives at the same phase from the same stored value by
// the same instructions.  The dt's a row pass applied WITHOUT storing are "retained" here; the stored phase is behind the handle's true phase
// by exactly them.  Whoever reads or replaces the stored phase flushes them first (ocean_capi.hip: flush_retained).

#pragma once

namespace ocean
{
  constexpr int MAX_PENDING = 8;      // dt's one row pass (or one launch of the phase-only kernel) applies

  struct PhaseWriteback
  {
    int retained = 0;                 // dt's applied by the last row pass and not stored
    float dt[MAX_PENDING] = {};       // ... oldest first

    // one row pass: the dt's it applies and whether it stores the phase
    struct Launch
    {
      int ndt = 0;
      float dt[MAX_PENDING] = {};
      bool store = false;
    };

    // whether a row pass can take the retained dt's and n newly queued ones in one list
    bool fits(int n) const { return retained + n <= MAX_PENDING; }

    // The row pass of a displace call with n newly queued dt's (fits(n); the caller brings the phase up to date otherwise) at a write-back
    // interval of `every` steps' worth of dt's (1 ... MAX_PENDING; 1 = every row pass that advances stores).  It stores when its list has
    // reached the interval -- a list of MAX_PENDING always has -- and retains the list otherwise.  n = 0 repeats the last row pass.
    Launch step(float const *pending, int n, int every)
    {
      Launch l;

      for(int i = 0; i < retained; ++i)
        l.dt[l.ndt++] = dt[i];

      for(int i = 0; i < n; ++i)
        l.dt[l.ndt++] = pending[i];

      l.store = l.ndt > 0 && l.ndt >= every;

      retained = l.store ? 0 : l.ndt;

      for(int i = 0; i < retained; ++i)
        dt[i] = l.dt[i];

      return l;
    }

    // the same list again, nothing stored and nothing changed (datum_ocean_debug_rowpass)
    Launch repeat() const
    {
      Launch l;

      for(int i = 0; i < retained; ++i)
        l.dt[l.ndt++] = dt[i];

      return l;
    }

    void clear() { retained = 0; }
  };
}
