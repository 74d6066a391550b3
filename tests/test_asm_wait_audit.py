"""The wait audit of csrc/Makefile (check_asm_waits.py, no GPU needed): every hand-written s_waitcnt waits for something, and every
inline-asm load is retired by a counted wait before its register is touched, on every path.  Synthetic assembly for each rule, the
k_fwd_ws counter handoff as it was compiled before its fix (lgkmcnt(15), a no-op), and the real forward unit cross-compiled for gfx950."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multiviewhmr_amd", "csrc")
SCRIPT = os.path.join(CSRC, "check_asm_waits.py")

WS = "_ZN5mvhmr8k_fwd_wsILi0ELi4EfLb1EEEvPK15HIP_vector_typeIfLj4EEPKfNS_6CoordsEPT1_iiiiiiiiiiiNS_4GateE"


def _mod():
    spec = importlib.util.spec_from_file_location("check_asm_waits", SCRIPT)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _asm(body, name=WS):
    return "%s:                ; @%s\n; %%bb.0:\n%s\ts_endpgm\n.Lfunc_end8:\n" % (name, name, body)


def _run(tmp_path, text, rules=("k_fwd_ws",)):
    p = tmp_path / "unit.s"
    p.write_text(text)
    return subprocess.run([sys.executable, SCRIPT] + list(rules) + ["--", str(p)], capture_output=True, text=True)


def _asm_block(*lines):
    return "\t;;#ASMSTART\n" + "".join("\t%s\n" % ln for ln in lines) + "\t;;#ASMEND\n"


TAPS8 = "".join("\tds_read_b128 v[%d:%d], v%d\n" % (4 * i, 4 * i + 3, 40 + i) for i in range(8))


def test_load_and_its_wait_in_one_asm_block_pass(tmp_path):
    r = _run(tmp_path, _asm(_asm_block("ds_read_b32 v83, v73", "s_waitcnt lgkmcnt(0)") + "\tv_readfirstlane_b32 s2, v83\n"))
    assert r.returncode == 0, r.stderr


def test_a_count_must_cover_exactly_the_younger_lds_reads(tmp_path):
    body = _asm_block("ds_read_b32 v83, v73") + TAPS8 + "%s" + "\tv_readfirstlane_b32 s2, v83\n"
    ok = _run(tmp_path, _asm(body % _asm_block("s_waitcnt lgkmcnt(8)")))
    assert ok.returncode == 0, ok.stderr
    bad = _run(tmp_path, _asm(body % _asm_block("s_waitcnt lgkmcnt(9)")))
    assert bad.returncode == 1 and "v83" in bad.stderr and "k_fwd_ws" in bad.stderr and "v_readfirstlane_b32 s2, v83" in bad.stderr
    # a compiler wait that happens to cover the load (its own count of the taps) retires it too
    comp = _run(tmp_path, _asm(_asm_block("ds_read_b32 v83, v73") + TAPS8 + "\ts_waitcnt lgkmcnt(7)\n\tv_mul_f32_e32 v1, v0, v2\n"
                               "\tv_readfirstlane_b32 s2, v83\n"))
    assert comp.returncode == 0, comp.stderr


def test_younger_smem_and_flat_operations_are_not_counted(tmp_path):
    # seven LDS reads + one scalar load behind the counter read: lgkmcnt(8) could be satisfied by the SMEM returning early
    seven = "".join("\tds_read_b128 v[%d:%d], v%d\n" % (4 * i, 4 * i + 3, 40 + i) for i in range(7))
    for younger in ("\ts_load_dwordx2 s[4:5], s[0:1], 0x0\n", "\tflat_load_dword v60, v[50:51]\n", "\ts_memtime s[6:7]\n"):
        r = _run(tmp_path, _asm(_asm_block("ds_read_b32 v83, v73") + seven + younger + _asm_block("s_waitcnt lgkmcnt(8)")
                                + "\tv_readfirstlane_b32 s2, v83\n"))
        assert r.returncode == 1 and "v83" in r.stderr, younger
    # LDS-DMA is vector memory: no LGKM count either
    r = _run(tmp_path, _asm(_asm_block("ds_read_b32 v83, v73") + seven + _asm_block("global_load_lds_dwordx4 v9, s[2:3]")
                            + _asm_block("s_waitcnt lgkmcnt(8)") + "\tv_readfirstlane_b32 s2, v83\n"))
    assert r.returncode == 1


def test_a_use_on_one_arm_of_a_diamond_fails(tmp_path):
    body = (_asm_block("ds_read_b32 v83, v73") + "\ts_cbranch_scc0 .LBB8_2\n"
            "; %bb.1:\n\tv_add_f32_e32 v1, v83, v1\n\ts_branch .LBB8_3\n"
            ".LBB8_2:\n\tv_mov_b32 v2, v1\n"
            ".LBB8_3:\n" + _asm_block("s_waitcnt lgkmcnt(0)") + "\tv_readfirstlane_b32 s2, v83\n")
    r = _run(tmp_path, _asm(body))
    assert r.returncode == 1 and "v83" in r.stderr and "%bb.1" in r.stderr
    # the same diamond with the use on neither arm passes
    ok = _run(tmp_path, _asm(body.replace("v_add_f32_e32 v1, v83, v1", "v_add_f32_e32 v1, v84, v1")))
    assert ok.returncode == 0, ok.stderr


def test_a_compiler_write_to_the_destination_before_the_wait_fails(tmp_path):
    r = _run(tmp_path, _asm(_asm_block("ds_read_b64 v[82:83], v73") + "\tv_mov_b32_e32 v83, 0\n" + _asm_block("s_waitcnt lgkmcnt(0)")
                            + "\tv_readfirstlane_b32 s2, v82\n"))
    assert r.returncode == 1 and "v83" in r.stderr and "v_mov_b32_e32 v83, 0" in r.stderr
    # AGPR destinations are registers too
    r = _run(tmp_path, _asm(_asm_block("ds_read_b64 a[0:1], v73") + "\tv_accvgpr_read_b32 v0, a1\n" + _asm_block("s_waitcnt lgkmcnt(0)")))
    assert r.returncode == 1 and "a1" in r.stderr


def test_a_load_pending_at_the_end_or_at_a_call_fails(tmp_path):
    r = _run(tmp_path, _asm(_asm_block("ds_read_b32 v83, v73") + "\ts_barrier\n\ts_sleep 1\n"))
    assert r.returncode == 1 and "s_endpgm" in r.stderr                   # barriers and sleeps retire nothing
    r = _run(tmp_path, _asm(_asm_block("ds_read_b32 v83, v73") + "\ts_swappc_b64 s[30:31], s[16:17]\n" + _asm_block("s_waitcnt lgkmcnt(0)")))
    assert r.returncode == 1 and "s_swappc_b64" in r.stderr


def test_vector_memory_loads_are_counted_in_issue_order(tmp_path):
    load = _asm_block("global_load_dword v5, v[0:1], off")
    younger = "\tbuffer_store_dwordx4 v[8:11], v2, s[4:7], 0 offen\n" + _asm_block("global_load_lds_dwordx4 v9, s[2:3]") + "\tflat_store_dword v[0:1], v3\n"
    ok = _run(tmp_path, _asm(load + younger + _asm_block("s_waitcnt vmcnt(2)") + "\tv_add_u32_e32 v6, v5, v5\n"))
    assert ok.returncode == 0, ok.stderr
    bad = _run(tmp_path, _asm(load + younger + _asm_block("s_waitcnt vmcnt(3)") + "\tv_add_u32_e32 v6, v5, v5\n"))   # flat_* does not count
    assert bad.returncode == 1 and "v5" in bad.stderr
    # an LDS wait does not retire a vector-memory load
    lgkm = _run(tmp_path, _asm(load + _asm_block("s_waitcnt lgkmcnt(0)") + "\tv_add_u32_e32 v6, v5, v5\n"))
    assert lgkm.returncode == 1


def test_the_walk_terminates_on_loops_and_joins_conservatively(tmp_path):
    # the load sits in a loop; the back edge carries it, still pending, to a use at the loop head
    body = (".LBB8_1:\n\tv_readfirstlane_b32 s3, v83\n" + _asm_block("ds_read_b32 v83, v73") + TAPS8
            + "\ts_cbranch_scc1 .LBB8_1\n" + _asm_block("s_waitcnt lgkmcnt(8)") + "\tv_mov_b32 v1, v83\n")
    r = _run(tmp_path, _asm(body))
    assert r.returncode == 1 and "v_readfirstlane_b32 s3, v83" in r.stderr
    # a loop that issues more LDS reads on one path only: the join keeps the smaller count, lgkmcnt(8) is then too weak
    body = (_asm_block("ds_read_b32 v83, v73") + "\ts_cbranch_scc1 .LBB8_3\n; %bb.2:\n" + TAPS8 + ".LBB8_3:\n"
            + "".join("\tds_read_b32 v%d, v%d\n" % (100 + i, 40 + i) for i in range(4)) + _asm_block("s_waitcnt lgkmcnt(8)")
            + "\tv_mov_b32 v1, v83\n")
    r = _run(tmp_path, _asm(body))
    assert r.returncode == 1 and "v83" in r.stderr


def test_a_hand_written_no_op_wait_fails(tmp_path):
    r = _run(tmp_path, _asm(_asm_block("ds_read_b32 v83, v73", "s_waitcnt lgkmcnt(0)") + _asm_block("s_waitcnt lgkmcnt(15)")))
    assert r.returncode == 1 and "no-op" in r.stderr and "lgkmcnt(15)" in r.stderr
    r = _run(tmp_path, _asm(_asm_block("ds_read_b32 v83, v73", "s_waitcnt lgkmcnt(0)") + _asm_block("s_waitcnt vmcnt(63) expcnt(7) lgkmcnt(15)")))
    assert r.returncode == 1 and "no-op" in r.stderr
    # a compiler wait outside the ASM blocks is not the audit's business; one field below its maximum is a wait
    ok = _run(tmp_path, _asm(_asm_block("ds_read_b32 v83, v73", "s_waitcnt vmcnt(63) lgkmcnt(0)") + "\ts_waitcnt lgkmcnt(15)\n"))
    assert ok.returncode == 0, ok.stderr


def test_the_audit_does_not_pass_vacuously(tmp_path):
    body = _asm_block("ds_read_b32 v83, v73", "s_waitcnt lgkmcnt(0)")
    r = _run(tmp_path, _asm(body, name="_ZN5mvhmr9k_renamedILi0EEEvPK"))
    assert r.returncode == 1 and "no function matching 'k_fwd_ws'" in r.stderr
    r = _run(tmp_path, _asm(_asm_block("s_waitcnt lgkmcnt(0)", "s_barrier")))
    assert r.returncode == 1 and "no inline-asm load" in r.stderr           # k_fwd_ws without its counter reads
    assert _run(tmp_path, _asm(_asm_block("s_waitcnt lgkmcnt(0)", "s_barrier")), ("k_fwd_ws:waits",)).returncode == 0
    r = _run(tmp_path, _asm("\tv_mov_b32 v1, v2\n"), ("k_fwd_ws:waits",))
    assert r.returncode == 1 and "no hand-written s_waitcnt" in r.stderr


# k_fwd_ws, softmax, fp32 volume, prescaled features: the R-buffer handoff of a two-unit compute wave as hipcc compiled it before the
# fix (unproject_brick_fwd_m0.hip, gfx950).  The counter read, the eight tap reads of views 0 and 1, the softmax's overflow branch,
# then wait_r_free's `s_waitcnt lgkmcnt(15)` -- no wait at all -- and the readfirstlane of the counter; v83 is reused for a float
# sample further down.
PRE_FIX_EXCERPT = """\
.LBB8_210:                              ; =>This Loop Header: Depth=1
	;;#ASMSTART
	ds_read_b32 v83, v73
	;;#ASMEND
	s_nop 0
	v_add_u32_e32 v0, 0, v39
	v_add_u32_e32 v1, 0, v40
	ds_read_b128 v[20:23], v0
	ds_read_b128 v[16:19], v1
	v_add_u32_e32 v0, v0, v32
	v_add_u32_e32 v1, v1, v32
	ds_read_b128 v[28:31], v0
	ds_read_b128 v[24:27], v1
	s_nop 0
	v_add_u32_e32 v8, 0, v48
	v_add_u32_e32 v9, 0, v49
	ds_read_b128 v[4:7], v8
	ds_read_b128 v[0:3], v9
	v_add_u32_e32 v8, v8, v41
	v_add_u32_e32 v9, v9, v41
	ds_read_b128 v[12:15], v8
	ds_read_b128 v[8:11], v9
	; sched_barrier mask(0x00000000)
	v_add_f32_e32 v100, v95, v93
	v_cmp_ngt_f32_e32 vcc, s5, v100
	s_cbranch_vccz .LBB8_212
; %bb.211:                              ;   in Loop: Header=BB8_210 Depth=1
	v_add_f32_e32 v87, v77, v87
	v_mul_f32_e32 v75, v75, v80
	s_branch .LBB8_213
.LBB8_212:                              ;   in Loop: Header=BB8_210 Depth=1
	v_mul_f32_e32 v87, v87, v98
	v_fmac_f32_e32 v75, v80, v89
.LBB8_213:                              ;   in Loop: Header=BB8_210 Depth=1
	;;#ASMSTART
	s_waitcnt lgkmcnt(15)
	;;#ASMEND
	s_branch .LBB8_215
.LBB8_214:                              ;   in Loop: Header=BB8_215 Depth=2
	s_andn2_b64 vcc, exec, s[2:3]
	s_cbranch_vccz .LBB8_217
.LBB8_215:                              ;   Parent Loop BB8_210 Depth=1
	v_readfirstlane_b32 s2, v83
	s_cmp_ge_i32 s2, s6
	s_mov_b64 s[2:3], -1
                                        ; implicit-def: $vgpr83
	s_cbranch_scc1 .LBB8_214
; %bb.216:                              ;   in Loop: Header=BB8_215 Depth=2
	s_sleep 1
	;;#ASMSTART
	ds_read_b32 v83, v73
	s_waitcnt lgkmcnt(0)
	;;#ASMEND
	s_mov_b64 s[2:3], 0
	s_branch .LBB8_214
.LBB8_217:                              ;   in Loop: Header=BB8_210 Depth=1
	;;#ASMSTART
	ds_write2st64_b32 v68, v77, v75 offset0:0 offset1:32
	;;#ASMEND
	s_waitcnt lgkmcnt(7)
	v_mul_f32_e32 v83, v112, v20
	s_cbranch_scc1 .LBB8_210
"""


def test_the_pre_fix_k_fwd_ws_handoff_fails(tmp_path):
    """regression test of the R-buffer handoff race: wait_r_free waited with lgkmcnt(15), the counter's maximum"""
    r = _run(tmp_path, _asm(PRE_FIX_EXCERPT))
    assert r.returncode == 1
    assert "k_fwd_ws" in r.stderr and "ds_read_b32 v83, v73" in r.stderr and "v83" in r.stderr
    assert "is a no-op" in r.stderr and "v_readfirstlane_b32 s2, v83" in r.stderr
    assert "LBB8_210 -> %bb.211 -> LBB8_213 -> LBB8_215" in r.stderr or "LBB8_210 -> LBB8_212 -> LBB8_213 -> LBB8_215" in r.stderr
    # the fixed count (4 LDS reads per view behind the counter read, two views) retires the read on both arms
    fixed = _run(tmp_path, _asm(PRE_FIX_EXCERPT.replace("s_waitcnt lgkmcnt(15)", "s_waitcnt lgkmcnt(8)")))
    assert fixed.returncode == 0, fixed.stderr


def test_the_forward_unit_passes_the_audit_in_its_isa(tmp_path):
    """cross-compile unproject_brick_fwd_m0.hip (k_fwd_ws, k_fwd_brick, k_fwd_brick_groups for the softmax) for gfx950 and audit it:
    every k_fwd_ws instance must hold its counter reads, and each must be retired by a counted wait before `seen` is read"""
    asm = tmp_path / "m0.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
                           "-fno-slp-vectorize", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(CSRC, "unproject_brick_fwd_m0.hip")], stderr=subprocess.DEVNULL)
    msgs, per_fn = _mod().audit([str(asm)], {"k_fwd_ws": "loads", "k_fwd_brick": "waits"})
    assert msgs == []
    ws = {n: v for n, v in per_fn.items() if "k_fwd_ws" in n}
    assert len(ws) == 6                                                     # fp32 / fp16 / bf16 volume x prescaled or not
    for name, (loads, waits) in ws.items():
        assert any(ld.startswith("ds_read_b32") for ld in loads), name
        assert waits > 0, name
