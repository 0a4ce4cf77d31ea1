// Host-only helpers shared by the launch planners (conv_plan.h, wgrad_plan.h) and, through common.h, by every translation unit.
// Nothing from HIP in here: the planners compile with a plain host compiler (tests/test_launch_plan_cpu.py).
#pragma once
#include "chap_hip.h"

void chap_set_error(const char* fmt, ...);
#define CHAP_CHECK_ARG(cond, ...) do { if (!(cond)) { chap_set_error(__VA_ARGS__); return CHAP_EINVAL; } } while (0)

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
