// Host-only check of cilantro_amd/csrc/loop_policy.hpp: the rules by which the ICP loops choose an iteration's kernel form.
// Every expected value follows from the integer products and strict comparisons of the rules themselves: no tolerance.
#include <cstdio>
#include <vector>

#include "../../cilantro_amd/csrc/loop_policy.hpp"

using namespace cilhip;

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); ++g_fail; } } while (0)

static const unsigned int NS = 1000000u;
static FbView view(unsigned int iterations, unsigned int unproven, unsigned int listed, float step) {
  return FbView{false, iterations, unproven, listed, 0.0f, 0.0f, step};
}

int main() {
  // the values other code reads (cilhip_get_last_run_trace, bench.py, the tests)
  CHECK(FORM_SEARCH == 0 && FORM_TILE_ONE_PASS == 1 && FORM_WARM_FIRST == 2 && FORM_WARM == 3 && FORM_LANE_FUSED == 4);
  CHECK(FORM_MASK == 0x7f && FORM_COUNTED == 0x80);

  {  // form_of: iteration 0 and an iteration beyond the trace are unknown
    const std::vector<unsigned char> trace = {trace_byte(FORM_SEARCH, true), trace_byte(FORM_WARM_FIRST, false)};
    CHECK(form_of(trace, 0u) == FORM_UNKNOWN && form_of(trace, 3u) == FORM_UNKNOWN);
    CHECK(form_of(trace, 1u) == (FORM_SEARCH | FORM_COUNTED) && form_of(trace, 2u) == FORM_WARM_FIRST);
    CHECK(form_counted(form_of(trace, 1u)) && !form_counted(form_of(trace, 2u)) && !form_counted(FORM_UNKNOWN));
    CHECK(form_is_warm(FORM_WARM) && form_is_warm(FORM_WARM_FIRST | FORM_COUNTED) && !form_is_warm(FORM_TILE_ONE_PASS) && !form_is_warm(FORM_UNKNOWN));
  }
  {  // a quarter of the queries searched: 250 000 keeps paying, 250 001 halves the bar and counts a strike; three strikes ban
    LoopPolicy p;
    p.begin_run(1.0f);
    CHECK(p.warm_keeps_paying(250000u, NS) && p.thresh == 1.0f && p.strikes == 0);
    CHECK(!p.warm_keeps_paying(250001u, NS) && p.thresh == 0.5f && p.strikes == 1 && !p.warm_banned);
    CHECK(!p.warm_keeps_paying(250001u, NS) && p.thresh == 0.25f && p.strikes == 2 && !p.warm_banned);
    CHECK(!p.warm_keeps_paying(250001u, NS) && p.thresh == 0.125f && p.strikes == 3 && p.warm_banned);
    // banned: never a candidate, and a warm published iteration does not turn the form on again
    CHECK(!p.candidate(false, 0.0f));
    p.decide(view(5, 0, 1, 0.0f), FORM_WARM, NS, true, false);
    CHECK(!p.on);
    // the ban outlives the run's own state
    p.begin_run(1.0f);
    CHECK(p.warm_banned && p.strikes == 0 && p.thresh == 1.0f && !p.on && p.judged == 0u);
  }
  {  // far / near: a sixteenth of the queries unproven, judged on cold tile forms only
    LoopPolicy p;
    CHECK(p.far_mode);
    p.note_unproven(FORM_TILE_ONE_PASS, 62500u, NS); CHECK(!p.far_mode);
    p.note_unproven(FORM_SEARCH | FORM_COUNTED, 62501u, NS); CHECK(p.far_mode);
    p.note_unproven(FORM_WARM, 0u, NS); CHECK(p.far_mode);            // a warm iteration counts something else there
    p.note_unproven(FORM_SEARCH, 62500u, NS); CHECK(!p.far_mode);
    p.note_unproven(FORM_WARM_FIRST, NS, NS); CHECK(!p.far_mode);
    p.note_unproven(FORM_LANE_FUSED, NS, NS); CHECK(!p.far_mode);
    p.note_unproven(FORM_UNKNOWN, NS, NS); CHECK(!p.far_mode);
  }
  {  // the cold iteration's forecast: an eighth of the queries
    const int counted = FORM_SEARCH | FORM_COUNTED;
    CHECK(LoopPolicy::forecast_ok(counted, 125000u, NS, true) && !LoopPolicy::forecast_ok(counted, 125001u, NS, true));
    CHECK(LoopPolicy::forecast_ok(counted, 125001u, NS, false));      // option warm_forecast off
    CHECK(LoopPolicy::forecast_ok(FORM_SEARCH, 125001u, NS, true));   // the iteration did not count
    CHECK(LoopPolicy::forecast_ok(FORM_UNKNOWN, 125001u, NS, true));
    LoopPolicy p;
    p.begin_run(1.0f);
    p.decide(view(3, 0, 125001u, 0.5f), counted, NS, true, false); CHECK(!p.on);
    p.decide(view(3, 0, 125000u, 0.5f), counted, NS, true, true); CHECK(!p.on);       // the caller's "blocked" flag
    p.decide(view(3, 0, 125000u, 1.0f), counted, NS, true, false); CHECK(!p.on);      // step == thresh: not worthwhile
    p.decide(view(3, 0, 125000u, 0.5f), counted, NS, true, false); CHECK(p.on);
    CHECK(p.judged == 0u && p.strikes == 0);                                          // a cold iteration is never judged
  }
  {  // strict bars
    LoopPolicy p;
    p.begin_run(0.25f);
    CHECK(!p.warm_worthwhile(0.25f) && p.warm_worthwhile(0.2499999f));
    CHECK(!p.candidate(false, 2.0f) && p.candidate(false, 1.9999999f));               // step == 8 * thresh is not a candidate
    CHECK(!p.candidate(true, 0.0f));                                                  // the run just fell out of the form
    p.on = true; CHECK(!p.candidate(false, 0.0f));
  }
  {  // a published iteration is judged once
    LoopPolicy p;
    p.begin_run(1.0f);
    p.on = true;
    const FbView fv = view(4, 0, 250001u, 0.1f);
    CHECK(p.judge(fv, FORM_WARM, NS) && !p.on && p.strikes == 1 && p.judged == 4u && p.thresh == 0.5f);
    p.on = true;
    CHECK(!p.judge(fv, FORM_WARM, NS) && p.on && p.strikes == 1);                     // the same one at the next look
    p.decide(fv, FORM_WARM, NS, true, false); CHECK(p.strikes == 1 && p.on);          // ... and at the look that decides (0.1 < 0.5)
    CHECK(!p.judge(view(5, 0, 250001u, 0.1f), FORM_TILE_ONE_PASS, NS) && p.judged == 4u);      // a cold one is not judged here
    p.on = false;
    CHECK(!p.judge(view(6, 0, 250001u, 0.1f), FORM_WARM, NS) && p.judged == 4u);      // nor anything while the form is off
    // the deciding look judges a warm iteration it has not seen: it falls, the form stays off
    p.decide(view(6, 0, 250001u, 0.1f), FORM_WARM, NS, true, false);
    CHECK(!p.on && p.strikes == 2 && p.judged == 6u);
  }
  {  // a warm published iteration with listed == 0 is not judged
    LoopPolicy p;
    p.begin_run(1.0f);
    p.decide(view(7, 0, 0u, 0.5f), FORM_WARM_FIRST, NS, true, true);
    CHECK(p.judged == 0u && p.strikes == 0 && p.on);                                  // ("blocked" concerns cold iterations only)
  }
  if (g_fail) { std::printf("%d FAILED\n", g_fail); return 1; }
  std::printf("ALL OK\n");
  return 0;
}
