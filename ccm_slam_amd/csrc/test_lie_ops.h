// test_lie_ops.h — TEST-ONLY: one entry to every function of ba_math.h / sim3_math.h that the optimisers share, and to the raw libm calls and operations they are
// made of.  lie_eval(op, in, out) reads up to 48 doubles and writes up to 40; out[39] is a flag word (ba_spd6_inv's return value, else 1).  It contains no
// arithmetic of its own: it loads, calls and stores.  test_hooks.hip runs it one lane per item on the device; tests/test_lie_math_cpu.py and
// tests/host/lie_check.cpp compile the same lines with g++, so device and host run one source.  tests/lie_reference.py lists the layouts (OPS).
#pragma once
#include "sim3_math.h"

enum LieOp {
  LIE_NORMALIZE = 0, LIE_QROT, LIE_MAP, LIE_Q_TO_R, LIE_R_TO_Q, LIE_OPLUS, LIE_OPLUS_FAST, LIE_HUBER, LIE_SYM3_INV, LIE_SPD6_INV,
  LIE_SIM3_EXP, LIE_SIM3_LOG, LIE_SIM3_MUL, LIE_SIM3_INV, LIE_SIM3_MAP, LIE_LU3,
  LIE_SIN, LIE_COS, LIE_SINCOS, LIE_EXP, LIE_LOG, LIE_ACOS, LIE_SQRT, LIE_RCP, LIE_DIV, LIE_FMA, LIE_N_OPS
};
constexpr int kLieIn = 48, kLieOut = 40, kLieFlag = 39;

// false: unknown op (nothing written)
BA_HD bool lie_eval(int op, const double* in, double* out) {
  double flag = 1.0;
  switch (op) {
    case LIE_NORMALIZE: { BaPose T = ba_load_pose(in); ba_normalize_rotation(T); ba_store_pose(out, T); break; }
    case LIE_QROT: { double r[3]; ba_qrot(in[0], in[1], in[2], in[3], in + 4, r); out[0] = r[0]; out[1] = r[1]; out[2] = r[2]; break; }
    case LIE_MAP: { const BaPose T = ba_load_pose(in); double r[3]; ba_map(T, in + 7, r); out[0] = r[0]; out[1] = r[1]; out[2] = r[2]; break; }
    case LIE_Q_TO_R: { const BaPose T = ba_load_pose(in); double R[9]; ba_q_to_R(T, R); for (int i = 0; i < 9; i++) out[i] = R[i]; break; }
    case LIE_R_TO_Q: {
      double m[9]; for (int i = 0; i < 9; i++) m[i] = in[i];
      BaPose T{0, 0, 0, 0, 0, 0, 0}; ba_R_to_q(m, T); out[0] = T.qx; out[1] = T.qy; out[2] = T.qz; out[3] = T.qw; break;
    }
    case LIE_OPLUS: { double u[6]; for (int i = 0; i < 6; i++) u[i] = in[i]; ba_store_pose(out, ba_oplus(u, ba_load_pose(in + 6))); break; }
    case LIE_OPLUS_FAST: { double u[6]; for (int i = 0; i < 6; i++) u[i] = in[i]; ba_store_pose(out, ba_oplus_fast(u, ba_load_pose(in + 6))); break; }
    case LIE_HUBER: { double r0, r1; ba_huber(in[0], in[1], r0, r1); out[0] = r0; out[1] = r1; break; }
    case LIE_SYM3_INV: { double a[6], r[6]; for (int i = 0; i < 6; i++) a[i] = in[i]; ba_sym3_inv(a, r); for (int i = 0; i < 6; i++) out[i] = r[i]; break; }
    case LIE_SPD6_INV: {   // Inv starts as the caller's out[0..35]: a false return must leave it untouched
      double A[36], Inv[36]; for (int i = 0; i < 36; i++) { A[i] = in[i]; Inv[i] = out[i]; }
      flag = ba_spd6_inv(A, Inv) ? 1.0 : 0.0; for (int i = 0; i < 36; i++) out[i] = Inv[i]; break;
    }
    case LIE_SIM3_EXP: { double u[7]; for (int i = 0; i < 7; i++) u[i] = in[i]; sim3_store(out, sim3_exp(u)); break; }
    case LIE_SIM3_LOG: { double r[7]; sim3_log(sim3_load(in), r); for (int i = 0; i < 7; i++) out[i] = r[i]; break; }
    case LIE_SIM3_MUL: sim3_store(out, sim3_mul(sim3_load(in), sim3_load(in + 8))); break;
    case LIE_SIM3_INV: sim3_store(out, sim3_inv(sim3_load(in))); break;
    case LIE_SIM3_MAP: { double r[3]; sim3_map(sim3_load(in), in + 8, r); out[0] = r[0]; out[1] = r[1]; out[2] = r[2]; break; }
    case LIE_LU3: {
      double W[9], t[3], x[3]; for (int i = 0; i < 9; i++) W[i] = in[i]; for (int i = 0; i < 3; i++) t[i] = in[9 + i];
      sim3_lu3_solve(W, t, x); out[0] = x[0]; out[1] = x[1]; out[2] = x[2]; break;
    }
    case LIE_SIN: out[0] = sin(in[0]); break;
    case LIE_COS: out[0] = cos(in[0]); break;
    case LIE_SINCOS: { double s, c; sincos(in[0], &s, &c); out[0] = s; out[1] = c; break; }
    case LIE_EXP: out[0] = exp(in[0]); break;
    case LIE_LOG: out[0] = log(in[0]); break;
    case LIE_ACOS: out[0] = acos(in[0]); break;
    case LIE_SQRT: out[0] = sqrt(in[0]); break;
    case LIE_RCP: out[0] = 1.0 / in[0]; break;
    case LIE_DIV: out[0] = in[0] / in[1]; break;
    case LIE_FMA: out[0] = fma(in[0], in[1], in[2]); break;
    default: return false;
  }
  out[kLieFlag] = flag;
  return true;
}
