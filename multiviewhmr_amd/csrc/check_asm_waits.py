#!/usr/bin/env python3
"""Build gate on the device assembly (hipcc -save-temps): the hand-counted waits of the brick kernels must retire what they guard.

The brick kernels step outside hipcc's wait insertion: inline-asm LDS / vector-memory loads, and hand-written `s_waitcnt` in place of
__syncthreads.  The compiler does not see an inline-asm load, so nothing but the hand-written count keeps its register from being
read (or overwritten) while the load is still in flight -- and a wrong count is still right whenever the data happen to be early.

  rule 1  every s_waitcnt inside an ASM block (;;#ASMSTART .. ;;#ASMEND) waits for something: at least one field below its gfx9
          maximum (vmcnt 63, expcnt 7, lgkmcnt 15; a field left out counts as its maximum).  lgkmcnt(15) alone is a no-op.
  rule 2  every inline-asm load with a register destination (ds_read*, ds_*_rtn*, global_ / buffer_ / scratch_ / flat_load* without
          lds) is retired before any instruction reads or writes one of its destination registers, on every path.  The walk follows
          labelled and fall-through blocks and s_branch / s_cbranch_* targets (labels inside ASM blocks included) and joins paths
          conservatively (the smallest count of younger operations seen at an instruction).  The gfx950 model:
            LDS load      s_waitcnt lgkmcnt(N) retires it iff N <= k, k = younger in-order LGKM operations issued since (ds_*).
                          Younger SMEM, s_memtime, s_sendmsg and flat_* may return out of order: they never add to k.
            vector load   the same with vmcnt; younger global_ / buffer_ / scratch_ loads, stores, atomics and LDS-DMA count, flat_*
                          does not.  A flat_* load needs both: its vmcnt and lgkmcnt(0).
            nothing else retires a load (barriers, s_sleep, branches do not); reaching a call, a return or s_endpgm with the load
            pending fails.
Rule 1 and rule 2 apply to every function of the files.  The prefixes say which kernels must be there, so that a rename cannot turn
the gate off:

usage: check_asm_waits.py <kernel-name-prefix>[:loads|:waits] [...] -- file.s [...]
  :loads (the default)  functions matching the prefix must exist and hold at least one inline-asm load
  :waits                functions matching the prefix must exist and hold at least one hand-written s_waitcnt
Exits non-zero on a violation (naming the function, the load, the register and the path) or when the gate would be vacuous."""
import re
import sys

VM_MAX, EXP_MAX, LGKM_MAX = 63, 7, 15
K_CAP = 64                                  # counts above every counter's range: the walk's lattice is finite

_REG_RANGE = re.compile(r"\b([va])\[(\d+):(\d+)\]")
_REG_ONE = re.compile(r"\b([va])(\d+)\b")
_LABEL = re.compile(r"^([.\w$]+):(?:\s|;|$)")
_WAIT_FIELD = re.compile(r"(vmcnt|expcnt|lgkmcnt)\((\d+)\)")


def regs_of(text):
    """the VGPRs / AGPRs an operand string names, as {('v', 83), ...}"""
    out = set()
    for kind, lo, hi in _REG_RANGE.findall(text):
        out.update((kind, r) for r in range(int(lo), int(hi) + 1))
    for kind, n in _REG_ONE.findall(_REG_RANGE.sub(" ", text)):
        out.add((kind, int(n)))
    return out


def reg_name(r):
    return "%s%d" % r


def parse_wait(operands):
    """s_waitcnt operands -> {'vm': n, 'exp': n, 'lgkm': n} (fields left out: their maximum)"""
    ops = operands.strip()
    if re.fullmatch(r"(0x[0-9a-fA-F]+|\d+)", ops):                             # the raw gfx9 encoding
        imm = int(ops, 0)
        return {"vm": (imm & 0xF) | (((imm >> 14) & 3) << 4), "exp": (imm >> 4) & 7, "lgkm": (imm >> 8) & 0xF}
    w = {"vm": VM_MAX, "exp": EXP_MAX, "lgkm": LGKM_MAX}
    for field, n in _WAIT_FIELD.findall(ops):
        w[{"vmcnt": "vm", "expcnt": "exp", "lgkmcnt": "lgkm"}[field]] = min(int(n), {"vmcnt": VM_MAX, "expcnt": EXP_MAX, "lgkmcnt": LGKM_MAX}[field])
    return w


def load_kind(mn, operands):
    """counters an inline-asm load with a register destination is pending on: None (not such a load), ('lgkm',), ('vm',) or both"""
    if mn.startswith("ds_read") or (mn.startswith("ds_") and "_rtn" in mn):
        return ("lgkm",)
    if re.match(r"(global|buffer|scratch)_load", mn) and "lds" not in mn and not re.search(r"\blds\b", operands):
        return ("vm",)
    if mn.startswith("flat_load") and "lds" not in mn:
        return ("vm", "lgkm")
    return None


def counts_lgkm(mn):
    """a younger operation that LDS retires in order with the load (SMEM / flat / messages may return out of order: not counted)"""
    return mn.startswith("ds_") and not mn.startswith(("ds_gws", "ds_ordered", "ds_nop"))


def counts_vm(mn):
    return re.match(r"(global|buffer|scratch|tbuffer)_(load|store|atomic)", mn) is not None


def is_terminal(mn):
    return mn in ("s_endpgm", "s_setpc_b64", "s_swappc_b64", "s_call_b64", "s_endpgm_saved") or mn.startswith("s_endpgm")


class Insn:
    __slots__ = ("line", "text", "mn", "ops", "asm", "block", "regs")

    def __init__(self, line, text, asm, block):
        self.line, self.text, self.asm, self.block = line, text, asm, block
        body = text.split(";", 1)[0].strip()
        parts = body.split(None, 1)
        self.mn = parts[0]
        self.ops = parts[1] if len(parts) > 1 else ""
        self.regs = regs_of(self.ops)


class Function:
    def __init__(self, name):
        self.name, self.insns, self.labels = name, [], {}

    def succ(self, i):
        ins = self.insns[i]
        if is_terminal(ins.mn):
            return []
        if ins.mn == "s_branch":
            return [self.labels.get(ins.ops.split()[0], -1)]
        nxt = [i + 1] if i + 1 < len(self.insns) else []
        if ins.mn.startswith("s_cbranch_"):
            return [self.labels.get(ins.ops.split()[0], -1)] + nxt
        return nxt


def parse(path):
    """the functions of one assembly file"""
    funcs, fn, asm, block = [], None, False, ""
    for ln, line in enumerate(open(path), 1):
        ls = line.strip()
        m = re.match(r"^(_Z\S+):", ls)
        if m and not ls.startswith(".L"):
            fn, asm, block = Function(m.group(1)), False, "entry"
            funcs.append(fn)
            continue
        if fn is None:
            continue
        if ls.startswith(".Lfunc_end"):
            fn = None
            continue
        if ls.startswith(";;#ASMSTART"):
            asm = True
            continue
        if ls.startswith(";;#ASMEND"):
            asm = False
            continue
        m = re.match(r"^; %bb\.(\d+):", ls)
        if m:
            block = "%bb." + m.group(1)
            continue
        if not ls or ls.startswith(";"):
            continue
        m = _LABEL.match(ls)
        if m:
            block = m.group(1).lstrip(".")
            fn.labels[m.group(1)] = len(fn.insns)
            continue
        if ls.startswith("."):                                                   # a directive
            continue
        fn.insns.append(Insn(ln, ls, asm, block))
    return funcs


def walk(fn, i0, kinds, dst):
    """rule 2 for the load at fn.insns[i0]: None when every path retires it first, else (reason, register or None, index, path)"""
    # state: (pending vm, k vm, pending lgkm, k lgkm); the join is OR on pending, min on k
    start = ("vm" in kinds, 0, "lgkm" in kinds, 0)
    best, prev, work = {}, {}, []

    def push(j, st, frm):
        if j < 0:
            return ("is pending at a branch to an unknown label", None, frm)
        old = best.get(j)
        new = st if old is None else (old[0] or st[0], min(old[1], st[1]), old[2] or st[2], min(old[3], st[3]))
        if new != old:
            best[j], prev[j] = new, frm
            work.append(j)
        return None

    for j in fn.succ(i0):
        bad = push(j, start, i0)
        if bad:
            return bad + (path_to(fn, prev, i0, bad[2]),)
    while work:
        i = work.pop()
        pv, kv, pl, kl = best[i]
        ins = fn.insns[i]
        hit = ins.regs & dst
        if hit:
            return ("is read or written by `%s` (line %d)" % (ins.text, ins.line), reg_name(sorted(hit)[0]), i, path_to(fn, prev, i0, i))
        if is_terminal(ins.mn):
            return ("is still pending at `%s` (line %d)" % (ins.text, ins.line), None, i, path_to(fn, prev, i0, i))
        if ins.mn == "s_waitcnt":
            w = parse_wait(ins.ops)
            if pv and w["vm"] <= kv:
                pv = False
            if pl and w["lgkm"] <= kl:
                pl = False
            if not (pv or pl):
                continue                                                         # retired on this path
        if counts_vm(ins.mn):
            kv = min(kv + 1, K_CAP)
        if counts_lgkm(ins.mn):
            kl = min(kl + 1, K_CAP)
        for j in fn.succ(i):
            if j < 0:
                return ("is pending at `%s` (line %d), whose target is no label of the function" % (ins.text, ins.line), None, i,
                        path_to(fn, prev, i0, i))
            push(j, (pv, kv, pl, kl), i)
    return None


def path_to(fn, prev, i0, i):
    """the blocks from the load to instruction i (the predecessor chain that last lowered the state)"""
    chain, seen = [], set()
    while i is not None and i != i0 and i not in seen:
        seen.add(i)
        chain.append(fn.insns[i].block)
        i = prev.get(i)
    chain.append(fn.insns[i0].block)
    chain.reverse()
    return [b for k, b in enumerate(chain) if k == 0 or b != chain[k - 1]]


def audit_function(fn):
    """-> (violations, inline-asm loads, hand-written waits)"""
    bad, loads, waits = [], [], 0
    for i, ins in enumerate(fn.insns):
        if not ins.asm:
            continue
        if ins.mn == "s_waitcnt":
            waits += 1
            w = parse_wait(ins.ops)
            if w["vm"] >= VM_MAX and w["exp"] >= EXP_MAX and w["lgkm"] >= LGKM_MAX:
                bad.append("wait audit: %s: `%s` (line %d, block %s) is a no-op: every field at its gfx9 maximum (vmcnt 63, expcnt 7, lgkmcnt 15)"
                           % (fn.name, ins.text, ins.line, ins.block))
            continue
        kinds = load_kind(ins.mn, ins.ops)
        if kinds is None:
            continue
        dst = regs_of(ins.ops.split(",")[0])
        if not dst:
            continue
        loads.append(ins)
        r = walk(fn, i, kinds, dst)
        if r:
            reason, reg, _, path = r
            bad.append("wait audit: %s: inline-asm load `%s` (line %d): %s %s before a wait retires the load; path %s"
                       % (fn.name, ins.text, ins.line, reg if reg else "/".join(reg_name(x) for x in sorted(dst)), reason, " -> ".join(path)))
    return bad, loads, waits


def audit(files, rules):
    """rules: {prefix: 'loads' | 'waits'} -> (messages, {function name: ([inline-asm loads], hand-written waits)}); no messages = pass"""
    msgs, per_fn = [], {}
    for path in files:
        for fn in parse(path):
            bad, loads, waits = audit_function(fn)
            msgs += bad
            per_fn[fn.name] = ([ins.text for ins in loads], waits)
    for prefix, need in rules.items():
        hits = {n: v for n, v in per_fn.items() if prefix in n}
        if not hits:
            msgs.append("wait audit: no function matching '%s' in %s -- the gate would be off" % (prefix, " ".join(files)))
        elif need == "loads" and not sum(len(v[0]) for v in hits.values()):
            msgs.append("wait audit: functions matching '%s' hold no inline-asm load -- the gate would be off" % prefix)
        elif need == "waits" and not sum(v[1] for v in hits.values()):
            msgs.append("wait audit: functions matching '%s' hold no hand-written s_waitcnt -- the gate would be off" % prefix)
    return msgs, per_fn


def main(argv):
    if "--" not in argv:
        sys.stderr.write(__doc__)
        return 2
    i = argv.index("--")
    rules = {}
    for a in argv[:i]:
        prefix, _, need = a.partition(":")
        if need not in ("", "loads", "waits"):
            sys.stderr.write("wait audit: unknown requirement '%s' in '%s'\n" % (need, a))
            return 2
        rules[prefix] = need or "loads"
    files = argv[i + 1:]
    msgs, _ = audit(files, rules)
    for m in msgs:
        sys.stderr.write(m + "\n")
    return 1 if msgs else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
