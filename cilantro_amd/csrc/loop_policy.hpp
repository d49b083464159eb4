// loop_policy.hpp -- which kernel form an ICP iteration takes (search only, tiled one pass, warm-started, ...): the decisions
// of cilhip_icp_run and of the sharded runs (cilhip_icp_partial_sums), once.  Plain C++17, no HIP: compiled by the host
// compiler for tests/cpp/test_loop_policy.cpp.  Everything here is integer arithmetic or a strict f32 comparison.
#pragma once

#include <cstddef>
#include <vector>

namespace cilhip {

// kernel forms of an iteration's search (+ accumulation): cilhip_get_last_form_timing
enum { FORM_SEARCH = 0, FORM_TILE_ONE_PASS = 1, FORM_WARM_FIRST = 2, FORM_WARM = 3, FORM_LANE_FUSED = 4 };
// cilhip_ctx::trace_form, one byte per enqueued iteration: the form, and bit 7 = this cold iteration counted the queries a warm-started one after it would have to search
constexpr int FORM_MASK = 0x7f;
constexpr int FORM_COUNTED = 0x80;
constexpr int FORM_UNKNOWN = -1;

// What the run's epilogues have published (Feedback): a consistent snapshot of the LATEST published iteration.
struct FbView { bool done; unsigned int iterations, unproven, listed; float delta, prev_delta, step; };

// the trace byte of published iteration `iterations` (1-based), FORM_UNKNOWN for iteration 0 or one the trace does not hold
inline int form_of(const std::vector<unsigned char>& trace, unsigned int iterations) {
  return (iterations >= 1 && iterations <= trace.size()) ? (int)trace[iterations - 1] : FORM_UNKNOWN;
}
inline bool form_is(int fo, int form) { return fo >= 0 && (fo & FORM_MASK) == form; }
inline bool form_is_warm(int fo) { return form_is(fo, FORM_WARM) || form_is(fo, FORM_WARM_FIRST); }
inline bool form_counted(int fo) { return fo >= 0 && (fo & FORM_COUNTED) != 0; }
inline unsigned char trace_byte(int form, bool counted) { return (unsigned char)(form | (counted ? FORM_COUNTED : 0)); }

// The warm-started form (k_warm) pays while the queries move little between iterations: a query is settled without any search as
// long as it has moved less than the MARGIN its last search left it (distance to the second nearest target point minus distance
// to the nearest, capped by the searched block's faces -- a good fraction of the target's point spacing, whatever the source is).
// The epilogue publishes how far any source point can have moved in the last update (IcpState::motion_step); a run enters the
// form when that falls below `thresh` (a fraction of a cell), and the kernel's own count of the queries it had to search
// corrects the guess: a quarter of them searched = one iteration through the cold form (whose searches leave fresh margins)
// and half the bar; three such falls and the run stays cold.
struct LoopPolicy {
  // ---- outlive a run: reset with the clouds they describe (a new source, a new or shared target)
  bool warm_banned = false;   // the warm-started form was seen not to pay on this cloud pair (too few queries settled by the table)
  bool far_mode = true;       // tiled ICP loop: the source is far from alignment (many unproven octant searches): search and
                              // accumulate in two passes (the search's 3x3x3 pass settles them in LDS) instead of one
  // ---- one run's (begin_run)
  float thresh = 0.0f;        // the bar for (re-)entering the warm-started form: the last update moved no source point by more than this
  int strikes = 0;            // warm iterations of the run that had to search a quarter of their queries
  bool on = false;            // the loop has been seen to move little: iterations run warm-started until one of them has to search too many of its queries
  unsigned int judged = 0;    // the last published iteration whose listed count has been judged

  void begin_run(float bar) { thresh = bar; strikes = 0; on = false; judged = 0; }

  // the form of the COLD iterations (one pass / two passes), from the last cold iteration's count of queries its octant stage
  // left open (a warm-started iteration counts something else there: the queries its own search took to the shells)
  void note_unproven(int fo, unsigned int unproven, unsigned int ns) {
    if (fo >= 0 && (fo & FORM_MASK) <= FORM_TILE_ONE_PASS) far_mode = (unsigned long long)unproven * 16ull > (unsigned long long)ns;
  }
  // a warm iteration was seen to search `listed` of its queries: keep going?
  bool warm_keeps_paying(unsigned int listed, unsigned int ns) {
    if ((unsigned long long)listed * 4ull <= (unsigned long long)ns) return true;
    thresh *= 0.5f;
    if (++strikes >= 3) warm_banned = true;
    return false;
  }
  bool warm_worthwhile(float step) const { return step < thresh; }
  // a warm-started published iteration's count is judged ONCE (the same one can be the latest at two consecutive looks): did the run just fall out of the form?
  bool judge(const FbView& fv, int fo, unsigned int ns) {
    if (!on || fv.iterations <= judged || !form_is_warm(fo)) return false;
    judged = fv.iterations;
    if (warm_keeps_paying(fv.listed, ns)) return false;
    on = false;
    return true;
  }
  // within reach of the warm-started form: worth waiting for the LATEST iteration's step (decide)
  bool candidate(bool fell, float step) const { return !on && !fell && !warm_banned && step < 8.0f * thresh; }
  // a cold iteration's own forecast: at most an eighth of the queries would have to be searched (bit FORM_COUNTED: it counted them)
  static bool forecast_ok(int fo, unsigned int listed, unsigned int ns, bool warm_forecast) {
    return !warm_forecast || !form_counted(fo) || (unsigned long long)listed * 8ull <= (unsigned long long)ns;
  }
  // ... after which the form may be entered (blocked: the caller's own reason not to -- cooperative searches leave no margin keys)
  bool cold_admits(const FbView& fv, int fo, unsigned int ns, bool warm_forecast, bool blocked) const {
    return forecast_ok(fo, fv.listed, ns, warm_forecast) && !blocked && warm_worthwhile(fv.step);
  }
  // The decision on the latest published iteration: a warm-started one's `listed` is the queries it had to search, a cold
  // one's (if it counted) the queries a warm-started iteration after it would have to.
  void decide(const FbView& fv, int fo, unsigned int ns, bool warm_forecast, bool blocked) {
    if (form_is_warm(fo)) {
      bool fell = false;
      if (fv.iterations > judged && fv.listed != 0u) { judged = fv.iterations; fell = !warm_keeps_paying(fv.listed, ns); }
      if (!fell && !warm_banned) on = warm_worthwhile(fv.step);
    } else {
      on = cold_admits(fv, fo, ns, warm_forecast, blocked);
    }
  }
};

}  // namespace cilhip
