"""Wall time of bowgpu_sort_by_col_sharded at 8 ranks (Int64 key + one Float64 column, device-resident, outputs allocated ONCE outside
the timed region) for three shapes of the frame - each rank a sorted series over the same range (full merge), each rank shuffled over
the whole range, ranged shuffled shards (no merge) - on as many distinct devices as the box has (ranks dealt round-robin) and on
one device with the id repeated.  The comparator, in the same run, is what the library offered before the call: bowgpu_append of the
shards on one device + bowgpu_sort_by_col.  From bowgpu_sort_by_col_sharded_info of the same calls: the splitter search alone (rounds
and the slowest rank's wall time of it), the merge rounds alone and the radix passes of the local sorts (device events, slowest
rank) - and the merge's time per round set against the local sort's time per pass over the same number of rows per rank.
One process; run it under a time limit:
    timeout -k 10 900 python scratch/sort_sharded_wall.py [rows per rank]
Warm-up call, then REPS timed calls: median.  Writes profiles/sort_sharded_wall.txt."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from bow_amd import capi

WORLD = 8
n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 12_500_000          # 8 ranks: 1e8 rows in all (< 2^31)
REPS = 5
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median_ms(fn, reps=REPS):
    fn(); capi.synchronize()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); capi.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    return sorted(wall)[len(wall) // 2]


def shapes(rng):
    total = WORLD * n
    yield "sorted series over the same range (full merge)", [np.sort(rng.integers(0, total, n, dtype=np.int64)) for _ in range(WORLD)]
    yield "shuffled over the whole range", [rng.integers(0, total, n, dtype=np.int64) for _ in range(WORLD)]
    yield "ranged shuffled shards (no merge)", [rng.permutation(n).astype(np.int64) + r * n for r in range(WORLD)]


def place(keys, ids):
    ranks = []
    for r, k in enumerate(keys):
        capi.set_device(ids[r])
        ts = capi.Column(capi.DeviceBuffer.from_numpy(k), None, capi.INT64, 0, n, 0)
        val = capi.Column(capi.DeviceBuffer.from_numpy(k.astype(np.float64)), None, capi.FLOAT64, 0, n, 0)
        ranks.append([ts, val])
    outs = []
    for r in range(WORLD):
        capi.set_device(ids[r])
        outs.append([capi.OutColumn(n, capi.DEVICE) for _ in range(2)])
    capi.set_device(0)
    return ranks, outs


per_round, per_pass = {}, {}
ndev = capi.device_count()
say("device: %s   devices: %d   ranks: %d   rows per rank: %d   host cores available: %d"
    % (capi.device_name(), ndev, WORLD, n, len(os.sched_getaffinity(0))))
layouts = [("one device, id repeated", [0] * WORLD)]
if ndev > 1:
    layouts.append(("%d distinct devices" % min(ndev, WORLD), [r % ndev for r in range(WORLD)]))
else:
    say("distinct devices: NOT TAKEN (one device on this box)")

for label, keys in shapes(np.random.default_rng(7)):
    say("\n%s" % label)
    for lname, ids in layouts:
        ranks, outs = place(keys, ids)

        def sharded():
            _, unchanged = capi.sort_by_col_sharded(ranks, 0, ids, outs=outs)
            assert not unchanged

        say("  sort_by_col_sharded, %-24s wall median %9.2f ms" % (lname + ":", median_ms(sharded)))
        info = capi.sort_by_col_sharded_info()                      # of the last timed call
        say("    splitter search alone: %d rounds, %.3f ms (slowest rank, wall: launches, read backs, barriers)" % (info.splitter_rounds, info.splitter_ms))
        say("    local sorts: %d radix passes, %.3f ms (slowest rank, kernels, the read of the key included)" % (info.sort_passes, info.local_sort_ms))
        say("    merge alone: %d rounds on %d destination ranks, %.3f ms (slowest rank, kernels, merge_init included)"
            % (info.merge_rounds, info.merged_ranks, info.merge_ms))
        if info.merge_rounds:
            per_round[(label, lname)] = info.merge_ms / info.merge_rounds
        if info.sort_passes:
            per_pass[(label, lname)] = info.local_sort_ms / info.sort_passes
        if info.merge_rounds and info.sort_passes:
            say("    one merge round / one radix pass over the same %d rows, same call: %.3f ms / %.3f ms = %.2f"
                % (n, per_round[(label, lname)], per_pass[(label, lname)], per_round[(label, lname)] / per_pass[(label, lname)]))
        if ids == [0] * WORLD:
            a_outs = [capi.OutColumn(WORLD * n, capi.DEVICE) for _ in range(2)]
            s_outs = [capi.OutColumn(WORLD * n, capi.DEVICE) for _ in range(2)]
            kern = {}

            def append_then_sort():
                capi.append(ranks, outs=a_outs)
                kern["append"] = capi.last_kernel_ms()
                _, unchanged = capi.sort_by_col([capi.out_as_column(o) for o in a_outs], 0, outs=s_outs)
                kern["sort"], kern["name"] = capi.last_kernel_ms(), capi.last_kernel_instance()
                assert not unchanged

            say("  bowgpu_append + bowgpu_sort_by_col on one device:   wall median %9.2f ms   (kernels: append %.2f ms, sort %.2f ms = %s)"
                % (median_ms(append_then_sort), kern["append"], kern["sort"], kern["name"]))
            # the sharded result is the one-device result
            at = 0
            for r in range(WORLD):
                for i in range(2):
                    assert capi.checksum64(outs[r][i].values, n) == capi.checksum64(s_outs[i].values, n, word_offset=at), (label, r, i)
                at += n
            del a_outs, s_outs
        del ranks, outs

say("\nmerge rounds against radix passes, %d rows per rank, one device with the id repeated:" % n)
one = "one device, id repeated"
pass_ms = [v for (lab, ln), v in per_pass.items() if ln == one]
for (lab, ln), v in per_round.items():
    if ln != one:
        continue
    if pass_ms:
        say("  %s: %.3f ms per merge round; a radix pass of a local sort of as many rows (shuffled shape): %.3f ms; ratio %.2f"
            % (lab, v, pass_ms[0], v / pass_ms[0]))
    else:
        say("  %s: %.3f ms per merge round; radix passes: NOT TAKEN (no shape ran one)" % (lab, v))
if not per_round:
    say("  NOT TAKEN (no shape merged)")
os.makedirs("profiles", exist_ok=True)
with open("profiles/sort_sharded_wall.txt", "w") as f:
    f.write("\n".join(lines) + "\n")
