"""The draw-and-count loop of the simulation table kernels is written once, in csrc/simulate_draw.h (draw_count_units): the kernels on it
are a policy and a thin wrapper.  csrc/simulate_txindel.hip shares the header's draw, bounds and constants but keeps a loop of its own:
on the shared loop its kernel's argument blocks left the compiler a 20-byte stack frame."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mural_amd", "csrc")
FILES = {"simulate.hip": "simulate_draw_kernel", "simulate_conseq.hip": "simulate_conseq_draw_kernel",
         "simulate_txstruct.hip": "simulate_txstruct_draw_kernel", "simulate_txindel.hip": "simulate_txindel_draw_kernel"}
ON_THE_SHARED_LOOP = ("simulate.hip", "simulate_conseq.hip", "simulate_txstruct.hip")


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def _definition(text, kernel):
    """The kernel's definition: from its name to the brace that closes its body."""
    at = text.index("void " + kernel + "(")
    depth, i = 0, text.index("{", at)
    for j in range(i, len(text)):
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[at:j + 1]
    raise AssertionError("unbalanced braces in " + kernel)


@pytest.mark.parametrize("name", sorted(FILES))
def test_every_simulation_file_includes_the_shared_header(name):
    assert '#include "simulate_draw.h"' in _read(name)


@pytest.mark.parametrize("name", ON_THE_SHARED_LOOP)
def test_the_draw_kernel_is_a_wrapper_of_the_shared_loop(name):
    body = _definition(_read(name), FILES[name])
    assert "draw_count_units<T>(" in body
    for own in ("philox4x32_10(", "atomicAdd(", "__ballot(", "rb * 16 + j"):
        assert own not in body, (name, own)
    assert len(body.splitlines()) <= 8, body


def test_the_table_path_calls_philox_in_the_header_alone():
    header = _read("simulate_draw.h")
    loop = header[header.index("void draw_count_units("):]
    assert loop.count("philox4x32_10(") == 1 and loop.count("atomicAdd(") == 1
    for name in ON_THE_SHARED_LOOP:
        text = _read(name)
        assert "atomicAdd(" not in text, name
        assert text.count("philox4x32_10(") == (1 if name == "simulate.hip" else 0), name      # (the mutation list's row_label)


def test_unit_blocks_is_defined_in_one_file():
    defined = [name for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".h", ".cpp"))
               and re.search(r"(#define|constexpr\s+int)\s+\w*_UNIT_BLOCKS\b", _read(name))]
    assert defined == ["simulate_draw.h"], defined
