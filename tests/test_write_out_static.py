"""
What the compiler made of the float32 stream-out (raster.hip: write_out_bits), read off the BUILT product with tools/opcode_histogram.py's parser:
hipcc cross-compiles, llvm-objdump disassembles, no GPU involved.

The headline launch is bound by vector-instruction issue, and its stream-out is two loops of the headline instantiation: the one whose word columns
are all whole and the one with the bounds check, each with a run of 93 global_store_dwordx4 in its own body.  On
the parent of the change that brought this test (counted with the same tool and the same flags in the same session) their own bodies held 626 and
573 full-rate VALU instructions per pass; 186 of them were v_mov_b32 that copied table entries, read in pairs across two CHANNELS, into the operand
of a store, which takes the entries of two INDICES.  Now the entries are read straight into the operand: 350 and 297.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

HEADLINE = 'raster_scene_bits_kernel<4, 3, float, SceneArgs, false, 3>'
#: full-rate VALU instructions in the own bodies of the two stream-out loops of HEADLINE on the parent commit, in address order
PARENT_FULL_RATE = (626, 573)


@pytest.fixture(scope='module')
def lib():
    from torchdrivesim_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native.LIB_PATH


@pytest.fixture(scope='module')
def stream_out_loops(lib):
    """the own bodies ([(address, opcode, text)]) of the loops of HEADLINE that hold the run of float4 stores, in address order"""
    import opcode_histogram as oh
    insts = oh.parse(oh.disassemble(lib, HEADLINE))
    _, every = oh.loops(insts)
    out = []
    for s, e in every:
        nested = [o for o in every if o != (s, e) and s <= o[0] and o[1] <= e]
        own = [insts[i] for i in range(s, e + 1) if not any(o[0] <= i <= o[1] for o in nested)]
        if sum(1 for _, op, _ in own if op == 'global_store_dwordx4') >= 90:
            out.append(own)
    assert len(out) == 2, f'{len(out)} loops with a run of float4 stores'
    return out


def registers(operand):
    m = re.fullmatch(r'v\[(\d+):(\d+)\]', operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r'v(\d+)', operand)
    return {int(m.group(1))} if m else set()


def test_fewer_vector_instructions_than_on_the_parent(stream_out_loops):
    import opcode_histogram as oh
    counts = tuple(sum(1 for _, op, text in own if oh.classify(op, text) == 'full') for own in stream_out_loops)
    print('full-rate VALU per pass in the stream-out loops:', counts, 'parent:', PARENT_FULL_RATE)
    assert all(c < p for c, p in zip(counts, PARENT_FULL_RATE)), (counts, PARENT_FULL_RATE)


def test_table_entries_go_from_the_lds_read_into_the_store(stream_out_loops):
    """every register of a float4 store's data operand was last written by the table's ds_read, not by a copy"""
    for own in stream_out_loops:
        stores = 0
        for i, (_, op, text) in enumerate(own):
            if op != 'global_store_dwordx4':
                continue
            stores += 1
            need = registers(text.split()[2].rstrip(','))
            assert len(need) == 4, text
            for _, wop, wtext in reversed(own[:i]):
                if wop.startswith(('s_', 'global_store', 'ds_write')) or not need:
                    continue
                hit = registers(wtext.split()[1].rstrip(',')) & need
                if hit:
                    assert wop.startswith('ds_read'), f'{wtext}  feeds  {text}'
                    need -= hit
            # (what is left was read in front of the loop's own body: the first stores of a pass)
        assert stores >= 90


def test_the_bit_plane_kernels_have_no_static_lds(lib):
    """pair_tab_read addresses the pair table from LDS address 0: the table is the first thing in the dynamic LDS, which starts at 0 only as long as
    the kernel has no static LDS"""
    import kernel_resources
    table = kernel_resources.kernel_table(lib)
    names = [k for k in table if re.match(r'raster_(scene|list)_bits_kernel<', k)]
    assert len(names) > 50
    for k in names:
        assert table[k]['group_segment_fixed_size'] == 0, (k, table[k])
