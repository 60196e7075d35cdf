// The switch table's storage, its one environment parse, and the per-thread scopes (switches.hpp has the rules).
#include "switches.hpp"

#include <cstdlib>

namespace nc {
namespace sw {

const Row kRows[kCount] = {
#define NC_SW_ROW(id, env, def, eclamp, sclamp, frozen) {#id, env, def, eclamp, sclamp, frozen},
    NC_SWITCH_TABLE(NC_SW_ROW)
#undef NC_SW_ROW
};

std::atomic<int> g_value[kCount];

namespace {
int clamp(Clamp c, int v) {
  switch (c) {
    case kBool: return v != 0;
    case kRange02: return v < 0 ? 0 : v > 2 ? 2 : v;
    case kTerms: return (v == 0 || v == 3) ? v : 2;
    case kGuard: return v == 2 ? 2 : v ? 1 : 0;
    case kP2dTerms: return (v == 1 || v == 2) ? v : 3;
    default: return v;  // kRaw
  }
}

int parse_env(const Row& r) {  // the one getenv of the library
  const char* text = r.env ? getenv(r.env) : nullptr;
  return text ? clamp(r.env_clamp, atoi(text)) : r.def;
}
struct Load {
  Load() { for (int i = 0; i < kCount; ++i) g_value[i].store(parse_env(kRows[i]), std::memory_order_relaxed); }
} g_load;

// per thread: how many scopes are open, how many of them are whole-network calls, and the sample of every row (-1: none; frozen rows only)
thread_local int t_depth = 0, t_net_depth = 0, t_force3 = 0;
thread_local int t_sample[kCount] = {
#define NC_SW_NONE(id, env, def, eclamp, sclamp, frozen) -1,
    NC_SWITCH_TABLE(NC_SW_NONE)
#undef NC_SW_NONE
};
void open_scope() {
  if (t_depth++ == 0)
    for (int i = 0; i < kCount; ++i)
      if (kRows[i].frozen) t_sample[i] = raw((Id)i);
}
void close_scope() {
  if (--t_depth == 0)
    for (int i = 0; i < kCount; ++i) t_sample[i] = -1;
}
}  // namespace

int get(Id id) {
  const int f = t_sample[id];
  return f >= 0 ? f : raw(id);
}
int set(Id id, int v) { return g_value[id].exchange(clamp(kRows[id].set_clamp, v), std::memory_order_relaxed); }

}  // namespace sw

SwitchScope::SwitchScope() { sw::open_scope(); }
SwitchScope::~SwitchScope() { sw::close_scope(); }
NetworkScope::NetworkScope() { ++sw::t_net_depth; sw::open_scope(); }
NetworkScope::~NetworkScope() { --sw::t_net_depth; sw::close_scope(); }
ForceTwoTerm::ForceTwoTerm() : prev_terms(sw::t_sample[sw::SPLIT_TERMS]) { sw::t_sample[sw::SPLIT_TERMS] = 2; ++sw::t_depth; }
ForceTwoTerm::~ForceTwoTerm() { sw::t_sample[sw::SPLIT_TERMS] = prev_terms; sw::close_scope(); }
ForceThreeTerm::ForceThreeTerm() { ++sw::t_force3; }
ForceThreeTerm::~ForceThreeTerm() { --sw::t_force3; }
bool force_three_term() { return sw::t_force3 != 0; }
bool h2_guard_can_flip() { return sw::get(sw::H2_GUARD) == 2 || (sw::get(sw::H2_GUARD) == 1 && sw::t_net_depth == 0); }

}  // namespace nc
