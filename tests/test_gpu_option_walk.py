"""Every option of cmf_set_option, every counter of cmf_get_counter / cmf_events_get_counter and every timed kernel name of
cmf_time_kernel is a row of a table (csrc/cmf_options.h, csrc/cmf_options.hip, kTimedKernels in csrc/cmf_api.hip).  The library is held,
cell for cell, to tests/golden/option_walk.json (tools/record_option_walk.py, recorded through the strcmp chains the tables replaced):
return codes and refusal texts, and behind every accepted value the bits of W, H and the losses of the next iterations with the launch
counters that produced them.  The walk is tests/option_walk.py; it makes 123 small handles and takes about a second."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "option_walk.json")


@pytest.fixture(scope="module")
def cmf():
    import cmf_jl_amd as m

    assert m.load_library().cmf_device_count() >= 1, "no HIP device: the gpu tests need a real MI355X"
    return m


def test_the_recorded_walk_cell_for_cell(cmf):
    import option_walk as walk

    with open(GOLDEN) as f:
        golden = json.load(f)["cells"]
    before = walk.handles_made
    cells = walk.walk()
    assert walk.handles_made - before == 123
    assert sorted(cells) == sorted(golden)  # (no cell is skipped, none is new)
    wrong = [(k, cells[k], golden[k]) for k in cells if cells[k] != golden[k]]
    assert not wrong, f"{len(wrong)} of {len(cells)} cells differ from the recording, first: {wrong[:5]}"
    # the recording itself: every section, every kind of handle, refusals among the accepted values
    for prefix in ("opt|few|", "opt|k32|", "opt|group|", "opt|shard|", "opt|hals|", "counter|few|", "counter|group|", "counter|events|",
                   "time|few|", "time|k32|", "time|group|", "profile|few|"):
        part = [v for k, v in golden.items() if k.startswith(prefix)]
        assert part and any(v[0] == 0 for v in part) and any(v[0] != 0 for v in part), prefix
