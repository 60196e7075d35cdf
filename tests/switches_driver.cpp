// Stand-alone driver of csrc/switches.cpp for tests/test_switches.py (host only: no HIP, no library).  One line per fact; the test asserts.
//   rows    ROW <identifier> <variable or -> <frozen 0|1> <value after load>     (the environment is the test's)
//   set     SET <identifier> <argument> <returned> <value afterwards>            (every row, arguments -3 .. 7 in a fixed order)
//   scope   CHECK <name> ok|FAIL                                                 (the scope rules, a second thread where one matters)
#include <cstdio>
#include <cstring>
#include <functional>
#include <thread>

#include "../neuroclear_amd/csrc/switches.hpp"

using namespace nc;

static int g_failed = 0;
static void check(const char* name, bool ok) {
  printf("CHECK %s %s\n", name, ok ? "ok" : "FAIL");
  if (!ok) ++g_failed;
}
// what "another thread moves the switch" means here: a thread that has no scope open, run to its end
static void elsewhere(const std::function<void()>& f) { std::thread(f).join(); }
static void set4(int terms, int guard, int fold, int stream) {
  sw::set(sw::SPLIT_TERMS, terms); sw::set(sw::H2_GUARD, guard); sw::set(sw::IN_BWD_FOLD, fold); sw::set(sw::STREAM_PASSES, stream);
}
static bool see4(int terms, int guard, int fold, int stream) {
  return sw::get(sw::SPLIT_TERMS) == terms && sw::get(sw::H2_GUARD) == guard && sw::get(sw::IN_BWD_FOLD) == fold && sw::get(sw::STREAM_PASSES) == stream;
}
// no slot holds a sample: whatever is set now is what get returns, for every frozen row
static bool all_clear() {
  bool ok = true;
  for (int i = 0; i < sw::kCount; ++i) {
    if (!sw::kRows[i].frozen) continue;
    for (int v : {0, 1}) { sw::set((sw::Id)i, v); ok = ok && sw::get((sw::Id)i) == sw::raw((sw::Id)i); }
  }
  return ok;
}

template <class Scope>
static void frozen_in(const char* tag) {
  char name[96];
  set4(2, 1, 1, 1);
  sw::set(sw::EPI_STATS, 1);
  {
    Scope sc;
    elsewhere([] { set4(3, 2, 0, 0); sw::set(sw::EPI_STATS, 2); });
    snprintf(name, sizeof name, "%s_keeps_frozen_rows", tag);
    check(name, see4(2, 1, 1, 1));
    snprintf(name, sizeof name, "%s_raw_moves", tag);
    check(name, sw::raw(sw::SPLIT_TERMS) == 3 && sw::raw(sw::H2_GUARD) == 2 && sw::raw(sw::IN_BWD_FOLD) == 0 && sw::raw(sw::STREAM_PASSES) == 0);
    snprintf(name, sizeof name, "%s_other_rows_live", tag);
    check(name, sw::get(sw::EPI_STATS) == 2);
    bool other = false;
    elsewhere([&] { other = see4(3, 2, 0, 0); });
    snprintf(name, sizeof name, "%s_is_per_thread", tag);
    check(name, other);
  }
  snprintf(name, sizeof name, "%s_closed_sees_now", tag);
  check(name, see4(3, 2, 0, 0));
  snprintf(name, sizeof name, "%s_closed_all_clear", tag);
  check(name, all_clear());
}

static void scopes() {
  frozen_in<SwitchScope>("switch_scope");
  frozen_in<NetworkScope>("network_scope");

  set4(2, 1, 1, 1);
  {
    SwitchScope outer;
    { NetworkScope inner; elsewhere([] { set4(3, 0, 0, 0); }); check("nested_inner_keeps", see4(2, 1, 1, 1)); }
    check("nested_inner_close_keeps", see4(2, 1, 1, 1));
    { SwitchScope again; check("nested_reopen_does_not_sample", see4(2, 1, 1, 1)); }
  }
  check("nested_outer_close_clears", see4(3, 0, 0, 0) && all_clear());

  // ForceTwoTerm outside a scope: the terms alone; the other rows stay live, also for a scope opened inside it
  set4(3, 1, 1, 1);
  {
    ForceTwoTerm f2;
    check("force2_outside_sees_two", sw::get(sw::SPLIT_TERMS) == 2 && sw::raw(sw::SPLIT_TERMS) == 3);
    elsewhere([] { set4(0, 2, 0, 0); });
    check("force2_outside_other_rows_live", see4(2, 2, 0, 0));
    { SwitchScope sc; elsewhere([] { set4(0, 0, 1, 1); }); check("force2_outside_inner_scope_does_not_sample", see4(2, 0, 1, 1)); }
    { ForceTwoTerm again; check("force2_nested", sw::get(sw::SPLIT_TERMS) == 2); }
    check("force2_nested_restores", sw::get(sw::SPLIT_TERMS) == 2);
  }
  check("force2_outside_restores", sw::get(sw::SPLIT_TERMS) == 0 && all_clear());

  // inside a scope: overrides the sample, puts it back, the scope clears at depth 0
  set4(3, 1, 1, 1);
  {
    SwitchScope sc;
    { ForceTwoTerm f2; check("force2_inside_sees_two", see4(2, 1, 1, 1)); }
    elsewhere([] { set4(0, 2, 0, 0); });
    check("force2_inside_restores_sample", see4(3, 1, 1, 1));
  }
  check("force2_inside_scope_close_clears", see4(0, 2, 0, 0) && all_clear());

  check("force3_off", !force_three_term());
  {
    ForceThreeTerm a;
    check("force3_on", force_three_term());
    { ForceThreeTerm b; check("force3_nested_on", force_three_term()); }
    check("force3_nested_close_still_on", force_three_term());
  }
  check("force3_closed_off", !force_three_term());
  bool other3 = true;
  { ForceThreeTerm a; elsewhere([&] { other3 = force_three_term(); }); }
  check("force3_is_per_thread", !other3);

  // h2_guard_can_flip: mode 2, or mode 1 outside a whole-network call
  const bool want_out[3] = {false, true, true}, want_net[3] = {false, false, true};
  for (int m = 0; m < 3; ++m) {
    char name[64];
    sw::set(sw::H2_GUARD, m);
    snprintf(name, sizeof name, "can_flip_mode%d_outside", m);
    check(name, h2_guard_can_flip() == want_out[m]);
    { SwitchScope sc; snprintf(name, sizeof name, "can_flip_mode%d_switch_scope", m); check(name, h2_guard_can_flip() == want_out[m]); }
    {
      NetworkScope net;
      snprintf(name, sizeof name, "can_flip_mode%d_network_scope", m);
      check(name, h2_guard_can_flip() == want_net[m]);
      { NetworkScope inner; }
      snprintf(name, sizeof name, "can_flip_mode%d_network_scope_after_inner", m);
      check(name, h2_guard_can_flip() == want_net[m]);
    }
    snprintf(name, sizeof name, "can_flip_mode%d_outside_again", m);
    check(name, h2_guard_can_flip() == want_out[m]);
  }
}

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!strcmp(mode, "rows")) {
    for (int i = 0; i < sw::kCount; ++i) {
      const sw::Row& r = sw::kRows[i];
      printf("ROW %s %s %d %d\n", r.name, r.env ? r.env : "-", r.frozen ? 1 : 0, sw::raw((sw::Id)i));
    }
    return 0;
  }
  if (!strcmp(mode, "set")) {
    for (int i = 0; i < sw::kCount; ++i)
      for (int v : {-3, -1, 0, 1, 2, 3, 5, 7}) {
        const int prev = sw::set((sw::Id)i, v);
        printf("SET %s %d %d %d\n", sw::kRows[i].name, v, prev, sw::raw((sw::Id)i));
      }
    return 0;
  }
  if (!strcmp(mode, "scope")) {
    scopes();
    return g_failed ? 1 : 0;
  }
  fprintf(stderr, "usage: switches_driver rows|set|scope\n");
  return 2;
}
