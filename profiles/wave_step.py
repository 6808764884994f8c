#!/usr/bin/env python3
"""Per wave-step figures of a GCM record kernel from a combine_pmc.py summary:
what one wave's step over 64 blocks costs the LDS array and the wave itself.

    python profiles/wave_step.py profiles/r07/pmc/prof_r07_c2_before.json <blocks-per-record>

A wave-step is 64 blocks, so a dispatch runs records x blocks / 64 of them.
The SQ wave counters (SQ_WAVE_CYCLES, SQ_ACTIVE_INST_*, SQ_WAIT_*) count in
units of 4 cycles: 4 x SQ_WAVE_CYCLES / waves is the dispatch's length in shader
cycles.  Prints JSON:
    lds_busy_cycles      SQ_LDS_IDX_ACTIVE per step (the LDS array's own cycles)
    wave_cycles          a wave's residency per step
    issue_cycles         ... of which it issued an instruction (SQ_ACTIVE_INST_ANY)
    valu_cycles, lds_issue_cycles   ... VALU / LDS instructions among those
    wait_issue_cycles    ... ready but not picked (SQ_WAIT_INST_ANY); wait_issue_lds_cycles: with an LDS
                         instruction next (SQ_WAIT_INST_LDS)
    waitcnt_cycles       ... in s_waitcnt (SQ_WAIT_ANY; the step loop waits on lgkmcnt only, but for one
                         vmcnt(0) a step behind its load)
    lds_busy_frac_resident   16 steps' LDS cycles over one wave's residency per step (16 waves per CU)
"""
import json
import sys

s = json.load(open(sys.argv[1]))
blocks = int(sys.argv[2])
sq1, sq2, sq3 = s["pmc_sq1"], s["pmc_sq2"], s["pmc_sq3"]
steps = s["derived"]["records_per_dispatch"] * blocks / 64
q = 4.0 / steps
out = {
    "wave_steps_per_dispatch": steps,
    "lds_busy_cycles": sq3["SQ_LDS_IDX_ACTIVE"] / steps,
    "wave_cycles": sq1["SQ_WAVE_CYCLES"] * q,
    "issue_cycles": sq2["SQ_ACTIVE_INST_ANY"] * q,
    "valu_cycles": sq2["SQ_ACTIVE_INST_VALU"] * q,
    "lds_issue_cycles": sq2["SQ_ACTIVE_INST_LDS"] * q,
    "wait_issue_cycles": sq2["SQ_WAIT_INST_ANY"] * q,
    "wait_issue_lds_cycles": sq1["SQ_WAIT_INST_LDS"] * q,
    "waitcnt_cycles": sq2["SQ_WAIT_ANY"] * q,
    "valu_insts": sq1["SQ_INSTS_VALU"] / steps,
    "lds_insts": sq1["SQ_INSTS_LDS"] / steps,
}
out["lds_busy_frac_resident"] = 16 * out["lds_busy_cycles"] / out["wave_cycles"]
out["lds_busy_frac"] = s["derived"]["lds_busy_frac"]
print(json.dumps({k: round(v, 4) if v < 10 else round(v, 1) for k, v in out.items()}, indent=1))
