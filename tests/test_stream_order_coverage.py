"""No device needed: every export of include/cnn_amd.h that takes a `void* stream` is placed -- in COVERED of tests/stream_order.py,
mapped to the test that runs it gated, or in EXEMPT with the reason why it queues no device work.  A new stream-taking export fails
here until it is placed."""
import os
import re

from tests import stream_order as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stream_taking_exports():
    """like tests/test_abi_exports.py::_declared_symbols, for the declarations with a `void* stream` parameter"""
    hdr = open(os.path.join(ROOT, "include", "cnn_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    found = re.findall(r"\b(cnn_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
    return sorted({name for name, params in found if re.search(r"\bvoid\s*\*\s*stream\b", params)})


def test_the_parser_finds_the_stream_taking_exports():
    names = _stream_taking_exports()
    assert len(names) >= 80
    for known in ("cnn_conv2d_backward", "cnn_relu_forward", "cnn_batch_stager_release", "cnn_amd_wait_published", "cnn_eval_read"):
        assert known in names
    for without in ("cnn_amd_side_stream_get", "cnn_batch_stager_submit", "cnn_conv2d_workspace_bytes", "cnn_stream_create"):
        assert without not in names


def test_every_stream_taking_export_is_placed():
    names = set(_stream_taking_exports())
    placed = set(SO.COVERED) | set(SO.EXEMPT)
    assert not (set(SO.COVERED) & set(SO.EXEMPT))
    assert sorted(names - placed) == [], "stream-taking exports without a gated test (COVERED) or a reason (EXEMPT)"
    assert sorted(placed - names) == [], "placed names that are no stream-taking export"
    assert all(isinstance(r, str) and r and "\n" not in r for r in SO.EXEMPT.values())


def test_covered_names_point_at_tests_that_exist():
    for name, test_id in SO.COVERED.items():
        path, _, func = test_id.partition("::")
        src = open(os.path.join(ROOT, path)).read()
        assert re.search(rf"^def {re.escape(func)}\(", src, flags=re.M), (name, test_id)


def test_case_tables_name_known_cases():
    """the tables beside the layer cases (bit-exact outputs, calls that block the host) speak of cases and outputs that exist"""
    from tests import stream_order_cases as K

    assert K.LAYER_BLOCKS <= set(K.LAYERS) and set(K.EXACT) <= set(K.LAYERS)
    for name, outputs in K.EXACT.items():
        inputs, reference = K.LAYERS[name]
        assert outputs <= set(reference(inputs())), name


def test_the_container_sequences_asked_for_exist():
    """every sequence on at least one net, every net under the default sequence; all of them device steps only"""
    from tests import host_layer_cases as L
    from tests.test_gpu_stream_order_container import CONTAINER_CASES, NETS, SEQUENCES

    assert {c.split("/")[1] for c in CONTAINER_CASES} == set(SEQUENCES)
    assert {c.split("/")[0] for c in CONTAINER_CASES} == set(NETS) and all(f"{n}/default" in CONTAINER_CASES for n in NETS)
    assert all(op[0] in ("step", "set") for c in CONTAINER_CASES for op in L.CASES[c][1])
