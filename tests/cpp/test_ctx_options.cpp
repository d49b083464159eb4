// test_ctx_options.cpp -- the option table of a context (csrc/ctx_options.hpp behind cilhip_set_option / cilhip_get_option), swept on the host:
// a cilhip_ctx constructed here takes both calls without any device.  For every row of the table and every value of the list below, set
// by key AND by id, plus keys and ids the table does not hold: one line with the return code, the read-back of ALL options, the four
// "something is stored" flags afterwards, and the error text.  The read-back is printed against the first line, which holds a fresh
// context's read-back in full: a case line names the options that read back differently from it, with their values ("-": none).  The two
// ways of setting share a line when they agree in everything, and get one each when they do not.  tests/test_cpp_host_api.py compares the
// output with tests/golden/option_sweep.txt byte for byte (recorded from this program linked against the library before the table moved).
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../cilantro_amd/csrc/ctx.hpp"

static std::vector<double> read_back(cilhip_ctx* c) {
  std::vector<double> v(cilhip_option_count(), NAN);
  for (int i = 0; i < (int)v.size(); ++i)
    if (cilhip_get_option(c, cilhip_option_info(i)->key, &v[i]) != CILHIP_OK) v[i] = NAN;
  return v;
}

static std::string run_case(const char* key, int id, bool by_id, double value, const std::vector<double>& fresh) {
  cilhip_ctx c;
  c.have_nn = c.pending_matches = c.have_pairs = c.has_src_grid = true;      // (inlier_fraction / one_to_one stay at their defaults)
  const int rc = by_id ? cilhip_set_option_id(&c, (cilhip_option)id, value) : cilhip_set_option(&c, key, value);
  const std::string err = c.err;
  char buf[256];
  snprintf(buf, sizeof(buf), "rc %d |", rc);
  std::string s = buf;
  const std::vector<double> now = read_back(&c);
  bool any = false;
  for (size_t i = 0; i < now.size(); ++i)
    if (!(now[i] == fresh[i])) { snprintf(buf, sizeof(buf), " %s=%.17g", cilhip_option_info((int)i)->key, now[i]); s += buf; any = true; }
  if (!any) s += " -";
  snprintf(buf, sizeof(buf), " | nn %d pending %d pairs %d src_grid %d | ", (int)c.have_nn, (int)c.pending_matches, (int)c.have_pairs, (int)c.has_src_grid);
  return s + buf + err;
}

int main() {
  const int n = cilhip_option_count();
  std::vector<double> fresh;
  { cilhip_ctx c; fresh = read_back(&c); }
  printf("fresh");
  for (int i = 0; i < n; ++i) printf(" %s=%.17g", cilhip_option_info(i)->key, fresh[i]);
  printf("\n");
  for (int id = 0; id < n; ++id) {
    const cilhip_option_info_t* o = cilhip_option_info(id);
    const double lo = o->min_value, hi = o->max_value;
    const std::vector<double> values = {o->default_value, lo, hi, lo - 1.0, hi + 1.0, 0.5 * (lo + hi), 0.5, 1.5, 2.5, 3.0, 5.0, 16.0, 1e-10, NAN};
    for (double v : values) {
      const std::string by_key = run_case(o->key, id, false, v, fresh), by_id = run_case(o->key, id, true, v, fresh);
      if (by_key == by_id) printf("key+id %s = %.17g -> %s\n", o->key, v, by_key.c_str());
      else printf("key %s = %.17g -> %s\nid %s = %.17g -> %s\n", o->key, v, by_key.c_str(), o->key, v, by_id.c_str());
    }
  }
  printf("key no_such_option = 1 -> %s\n", run_case("no_such_option", -1, false, 1.0, fresh).c_str());
  printf("id -1 = 1 -> %s\n", run_case("", -1, true, 1.0, fresh).c_str());
  printf("id %d = 1 -> %s\n", n, run_case("", n, true, 1.0, fresh).c_str());
  return 0;
}
