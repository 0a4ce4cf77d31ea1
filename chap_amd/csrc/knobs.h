// Every CHAP_* runtime knob of libchap_hip.so, declared ONCE: name, parse rule, default, liveness.  Nothing else in csrc reads the environment.
// (Host-only, no HIP: the launch planners that read most of these compile with a plain host compiler.)
//
// Parse rules
//   ANY   set -> atol(value), whatever it gives (0 and negative numbers are values); unset -> default
//   POS   set to a number > 0 -> that number; unset, 0, negative or not a number -> default
//   SET   1 when the variable exists, whatever it holds; 0 otherwise
//   TEXT  free text, read with chap_knob_text() (always live)
// Liveness
//   LIVE  re-read on every call: the tests, tools/shape_table.py sweeps and bench.py flip these inside one process
//   ONCE  read at first use, then fixed for the life of the process (one cache per knob for the whole library)
#pragma once
#include <atomic>
#include <cstdlib>

//    name (after CHAP_)    rule  default  liveness
#define CHAP_KNOBS(X) \
    /* conv_plan.h: routing and blocking of chap_conv_fwd */ \
    X(CONV_WP,              ANY,  1,       LIVE)  /* wave-private 2D kernels: 0 = never, N = from N tiles of 4 x 16 pixels up */ \
    X(CONV_KPAR,            ANY,  2,       LIVE)  /* K-parallel kernels: 0 = never, 1 = whenever eligible, 2 = 3D, by the block count */ \
    X(CONV_KPAR_MAX,        ANY,  800,     LIVE)  /* ... the block-count threshold of mode 2 */ \
    X(CONV_NT,              POS,  0,       LIVE)  /* override NT of the k3 s1 layers with >= CHAP_CONV_MINC input channels (0 = heuristics) */ \
    X(CONV_MR,              POS,  0,       LIVE)  /* ... and MR */ \
    X(CONV_MINC,            ANY,  64,      LIVE) \
    X(CONV_KC16_MAXC,       POS,  1 << 20, ONCE)  /* 3D 3x3x3: 16-channel chunks up to this many K channels (the packer and the conv share it) */ \
    X(CONV_KC16_MAXC2D,     POS,  0,       ONCE)  /* the same for 2D 3x3 */ \
    /* conv launchers */ \
    X(CONV_WP_BPC,          POS,  0,       LIVE)  /* wave-private blocks per CU (0 = 4 with 16-channel chunks, 2 with 32) */ \
    X(CONV_OCC_CAP,         POS,  0,       ONCE)  /* blocks per CU of the persistent grid (0 = 2 in 2D, whatever fits in 3D) */ \
    X(CONV_WLDS_KB,         POS,  0,       ONCE)  /* LDS budget of resident weights (0 = 100 KB in 2D, 158 in 3D) */ \
    /* wgrad_plan.h */ \
    X(WGRAD_WP,             ANY,  1,       LIVE)  /* wave-private 2D kernels: 0 = never, N = from N tiles of 8 x 16 pixels up */ \
    X(WGRAD_WP_MR,          ANY,  2,       LIVE)  /* ... their tile rows per wave = 4 * MR: 1, anything else = 2 */ \
    X(WGRAD_BRICK,          ANY,  16,      LIVE)  /* 3D bricks: 0 = slabs everywhere, N = from N bricks up */ \
    X(WGRAD_BLOCKS,         POS,  0,       LIVE)  /* split target of every layer (0 = per-class targets) */ \
    X(WGRAD_BRICK_BLOCKS,   POS,  256,     LIVE)  /* split target of the 3D bricks with 32-wide B tiles */ \
    X(WGRAD_WP_BLOCKS,      POS,  512,     ONCE)  /* split target of the wave-private kernels */ \
    X(WGRAD_TARGETS,        TEXT, 0,       LIVE)  /* "a,b,c": split targets of three layer classes (wgrad_plan.h) */ \
    X(WGRAD_BN16_MAXC,      POS,  16,      ONCE)  /* 3D bricks: 16-wide B tiles up to this many B channels */ \
    /* pointwise kernels */ \
    X(C1_MFMA,              ANY,  1,       ONCE)  /* 0 = the scalar one-input-channel conv */ \
    X(ACTBWD_BLOCKS,        POS,  512,     ONCE) \
    X(GRID_SCALE,           POS,  100,     ONCE)  /* per cent: scales the block cap of every grid-stride streaming kernel */ \
    /* chap_lab_skip(): timing bounds that skip every launch of a kind (wrong numerics), compiled into lab builds (-DCHAP_LAB) only */ \
    X(LAB_SKIP_BNFIN,       SET,  0,       ONCE) \
    X(LAB_SKIP_POOL,        SET,  0,       ONCE) \
    X(LAB_SKIP_UPSAMPLE,    SET,  0,       ONCE) \
    X(LAB_SKIP_UPSAMPLE_BWD, SET, 0,       ONCE) \
    X(LAB_SKIP_ACTSUM,      SET,  0,       ONCE) \
    X(LAB_SKIP_ACTAPPLY,    SET,  0,       ONCE)

enum chap_knob_rule { CHAP_KNOB_ANY, CHAP_KNOB_POS, CHAP_KNOB_SET, CHAP_KNOB_TEXT };
enum chap_knob_life { CHAP_KNOB_LIVE, CHAP_KNOB_ONCE };
#define CHAP_KNOB_ID(n, rule, def, life) KNOB_##n,
enum chap_knob_id { CHAP_KNOBS(CHAP_KNOB_ID) CHAP_KNOB_COUNT };
#undef CHAP_KNOB_ID
struct chap_knob_decl { const char* name; chap_knob_rule rule; long def; chap_knob_life life; };
#define CHAP_KNOB_ROW(n, rule, def, life) {"CHAP_" #n, CHAP_KNOB_##rule, def, CHAP_KNOB_##life},
inline constexpr chap_knob_decl chap_knob_table[CHAP_KNOB_COUNT] = {CHAP_KNOBS(CHAP_KNOB_ROW)};
#undef CHAP_KNOB_ROW

inline const char* chap_knob_text(chap_knob_id id) { return getenv(chap_knob_table[id].name); }

inline long chap_knob(chap_knob_id id) {
    static std::atomic<bool> have[CHAP_KNOB_COUNT];
    static std::atomic<long> value[CHAP_KNOB_COUNT];
    const chap_knob_decl& k = chap_knob_table[id];
    if (k.life == CHAP_KNOB_ONCE && have[id].load(std::memory_order_acquire)) return value[id].load(std::memory_order_relaxed);
    const char* e = chap_knob_text(id);
    long v = k.def;
    if (k.rule == CHAP_KNOB_SET) v = e ? 1 : 0;
    else if (e && (k.rule == CHAP_KNOB_ANY || atol(e) > 0)) v = atol(e);
    if (k.life == CHAP_KNOB_ONCE) { value[id].store(v, std::memory_order_relaxed); have[id].store(true, std::memory_order_release); }
    return v;
}

#ifdef CHAP_LAB
inline bool chap_lab_skip(chap_knob_id id) { return chap_knob(id) != 0; }
#else
inline bool chap_lab_skip(chap_knob_id) { return false; }
#endif
