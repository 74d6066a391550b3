#!/usr/bin/env python3
"""Build gate: kernels that pipeline LDS-DMA behind hand-counted `s_waitcnt vmcnt(N)` must not touch scratch --
a register spill is a vector-memory operation, is counted in vmcnt, and silently breaks the count.
Reads hipcc's -Rpass-analysis=kernel-resource-usage output.

k_fwd_brick is held to zero scratch here, and so is k_bwd_geom: it holds 3 V values per channel of a lane in registers (the
channels per lane shrink with V to keep that at <= 48), and a spill inside its channel loop would cost a scratch round trip per tap.  k_fwd_brick_groups and k_bwd_brick keep a cold noinline slow path whose call frame is
scratch OUTSIDE their hot loops; their loops are checked on the device assembly instead (check_loops.py).  k_bwd_brick's one
counted wait, wait_vmcnt(n_at) after the flush atomics, relies on vmcnt retiring in issue order: an extra vector-memory operation
the compiler adds among the wave's youngest could only make that wait cover more, never less.

The soft-argmax kernels (k_sa3d_*) stream the volume once with up to 20 accumulators and 24 coordinates live per lane: a spill would add
scratch traffic to a kernel whose whole budget is one read of the volume, so they are held to zero scratch too.

The volume-sampling kernels (k_vs3d_*) keep a point's eight tap offsets and weights, and up to 32 tap values, in registers while dozens of
gather loads are in flight: scratch traffic would queue behind those loads, so they are held to zero scratch as well.

The peak kernels (k_pk3d_*) keep a ring of up to 7 planes of box maxima, 4 voxels each, and the next plane's loads in registers, all
indexed statically: a ring that fell into scratch would turn one read of the volume into several, so they are held to zero scratch.

The projection kernels (k_pv3d_*) carry up to three accumulators for each of a block's eight channels across the whole march of a ray,
beside a sample's taps and 32 tap values in flight: an accumulator in scratch would be read and written once per sample and channel, so
they are held to zero scratch."""
import re
import sys

NO_SCRATCH = ("k_fwd_brick", "k_bwd_geom", "k_sa3d", "k_vs3d", "k_pk3d", "k_pv3d")
EXEMPT = re.compile(r"k_fwd_brick_groups")      # (k_fwd_ws: cold noinline slow path + prologue spills outside its loops; check_loops.py holds the loops)
text = open(sys.argv[1]).read()
bad = []
for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", text, flags=re.S):
    name, scratch = m.group(1), int(m.group(2))
    if any(k in name for k in NO_SCRATCH) and scratch and not EXEMPT.search(name):
        bad.append((name, scratch))
for name, scratch in bad:
    sys.stderr.write("resource check: %s uses %d bytes/lane of scratch (spills break counted vmcnt waits)\n" % (name, scratch))
sys.exit(1 if bad else 0)
