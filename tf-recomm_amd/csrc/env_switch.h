// env_switch.h - the one place that reads the environment.  Every TFR_* switch is an A/B or diagnostic knob (the table in
// DESIGN §23 lists them all); each follows one of three conventions, one reader each:
//     env_default_off(name)   on only where the value starts with '1'
//     env_default_on(name)    on unless the value starts with '0'
//     env_int(name, dflt)     an integer; dflt where unset
// A reader looks at the environment at every call.  A switch that is read once keeps the answer in a `static const` at
// its site (set on first use); the few that must follow a process that changes its environment call the reader
// each time.  A switch that two files read has its accessor here, so both see one answer.
#pragma once
#include <stdlib.h>

namespace tfr {

inline bool env_is_set(const char* name) { return getenv(name) != nullptr; }
inline bool env_default_off(const char* name) { const char* e = getenv(name); return e && e[0] == '1'; }
inline bool env_default_on(const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); }
inline long long env_int(const char* name, long long dflt) { const char* e = getenv(name); return e ? atoll(e) : dflt; }

// read by the step (api.hip), by launch_seg_reduce (svd_kernels.h: seg_reduce_pick) and by tfr_kernel_plan
inline bool switch_dualq() { static const bool on = env_default_on("TFR_DUALQ"); return on; }   // TFR_DUALQ=0: the big-table step copies the pre-update item rows (one table)
inline bool switch_fast() { static const bool on = env_default_on("TFR_FAST"); return on; }     // TFR_FAST=0: k_seg_reduce's general form everywhere
inline bool switch_lean() { static const bool on = env_default_on("TFR_LEAN"); return on; }     // TFR_LEAN=0: own row kept in registers
// read by the step (api.hip radix_sort_columns, run_train_step) and by tfr_kernel_plan
inline bool switch_rsort_wide() { static const bool on = env_default_on("TFR_RSORT_WIDE"); return on; }     // TFR_RSORT_WIDE=0: the 1024-key radix pass at every size
inline bool switch_tile_split() { static const bool on = env_default_off("TFR_TILE_SPLIT"); return on; }   // TFR_TILE_SPLIT=1: the three-launch small-table step (k_front + k_seg_reduce), kept for A/B

}  // namespace tfr
