"""Child process of tests/test_gpu_middle_paths.py: hits the kernel of pc_middle_paths must refuse.  Every one of them is
caught by a check the lane makes BEFORE it touches the arena, the interval table, the scratch or its outputs: an adapter index
outside the table (above it and negative), a read end outside [0, read_len], a negative mask count, a mask run that leaves
the n rows of the interval table, and a read longer than max_len.  The refused hits' outputs stay as they were, every other
hit of the call gets what a clean call gives it, and pc_sync reports the error once.

    python -m tests.middle_paths_child   ->   MIDDLE_PATHS_BAD_OK"""
import numpy as np


def main():
    import torch
    import porechop_amd
    from oracle.oracle import Oracle
    from tests import middlegen as mg
    from tests.test_gpu_middle_paths import MAX_LEN, device_inputs

    cases = mg.Cases(Oracle())
    hits = cases.hits("default")[:128]
    al = porechop_amd.Aligner(cases.adapters, mg.SCHEMES["default"])
    inputs = device_inputs(cases, hits)
    good = [x.cpu().numpy() for x in al.middle_paths(max_len=MAX_LEN, **inputs)]
    al.sync()
    bad = {k: v.clone() for k, v in inputs.items()}
    bad["adapter_idx"][5] = len(cases.adapters)
    bad["adapter_idx"][70] = -1
    bad["read_end"][6] = bad["read_len"][6] + 1
    bad["read_end"][7] = -1
    bad["mask_count"][8] = -1
    bad["mask_base"][9] = len(hits)
    bad["mask_count"][9] = 1                                          # one row behind the table
    bad["mask_base"][10] = -1
    longest = int(np.argmax([cases.length[h.read] for h in hits]))
    refused = [5, 6, 7, 8, 9, 10, 70]
    assert longest not in refused and cases.length[hits[longest].read] == MAX_LEN
    recs, heads, ops = al.middle_paths(max_len=MAX_LEN, **bad)
    try:
        al.sync()
    except RuntimeError:
        pass
    else:
        raise AssertionError("pc_sync reported nothing")
    got = [x.cpu().numpy() for x in (recs, heads, ops)]
    keep = np.array([k not in refused for k in range(len(hits))])
    for g, w in zip(got, good):
        assert np.array_equal(g[keep], w[keep]) and not g[~keep].any()
    # a read above max_len: the same call with max_len one below the longest read
    pitch = int(good[2].shape[1])
    recs, heads, ops = al.middle_paths(max_len=MAX_LEN - 1, ops_pitch=pitch, **inputs)
    try:
        al.sync()
    except RuntimeError:
        pass
    else:
        raise AssertionError("pc_sync reported nothing for a read above max_len")
    assert not recs.cpu().numpy()[longest].any() and not heads.cpu().numpy()[longest].any() and not ops.cpu().numpy()[longest].any()
    al.sync()                                                        # (the error word was cleared)
    al.close()
    print("MIDDLE_PATHS_BAD_OK")


if __name__ == "__main__":
    main()
