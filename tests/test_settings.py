"""grappa_amd/settings.py: the one table of engine settings, the one reader of the environment, and the stamp that both kinds of recorded
hipGraph (capture.CapturedForward, trainer.Trainer) derive from it.  CPU only: a real `HipBackend` is built over the recorder stub of
test_dense_front_end_trace.py (which clears GRAPPA_* from the environment first)."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from test_dense_front_end_trace import _Cx
from test_host_train import TINY

from grappa_amd import _lib, backend, ops, settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# typed from HipBackend.__init__, ops.py and ParameterWriter.__init__ of the commit before the table existed: the table must not move a default
BACKEND_DEFAULTS = dict(
    gemm_precision_name="f32_f16x3", gemm_precision=_lib.GEMM_PRECISIONS["f32_f16x3"], gemm_precision_bwd_name=None, gemm_precision_bwd=None,
    defer_wgrads=True, defer_ln=True, wgrad_queue_bytes=12 * 2 ** 30, inference_pairs=True, training_pairs=True, group_launches=True,
    amax_parts=False, fuse_ln_drop=True, pairs_min_rows=12288, backward_pairs=False, weight_pairs_min_rows=24000, _tails=None,
    plan_override=None, splitk_reduce=0, _tails_pinned=False, gnn_tails=False, wgrads_aside=True, weight_planes=False, fused_writer_layer=True,
    fused_writer_layer_bwd=True, fused_first_layer=True, first_layer_indexed=True, wgrad_column_maxima=False)
WRITER_DEFAULTS = dict(head_streams=4, merged_heads="0", merged_heads_max_tokens=40000)
FLAGS = [e for e in settings.TABLE if e.kind == "flag" and e.env]


def _same(a, b):
    return type(a) is type(b) and a == b


def _other(v):
    """a value that differs from v (any type will do: the stamp compares, nothing launches)"""
    return (not v) if isinstance(v, bool) else v + 1 if isinstance(v, int) else "another"


# ---- coverage
def test_every_environment_variable_named_in_the_package_and_the_tools_is_in_the_table():
    """a GRAPPA_* token counts as read or assigned where it stands in an environ / getenv expression or in front of `=` (a shell assignment, an
    `export`, the usage line of a docstring)"""
    envs = {e.env for e in settings.TABLE if e.env}
    files = (glob.glob(os.path.join(ROOT, "grappa_amd", "**", "*.py"), recursive=True) + glob.glob(os.path.join(ROOT, "tools", "*.py"))
             + glob.glob(os.path.join(ROOT, "tools", "*.sh")))
    assert len(files) > 40
    unknown = []
    for path in files:
        with open(path, encoding="utf-8") as f:
            for no, line in enumerate(f, 1):
                for m in re.finditer(r"GRAPPA_[A-Z_]+", line):
                    used = line[m.end():m.end() + 1] == "=" or re.search(r"environ[.\[]|getenv\(", line)
                    if used and m.group() not in envs:
                        unknown.append(f"{os.path.relpath(path, ROOT)}:{no}: {m.group()}")
    assert not unknown, unknown


def test_the_package_reads_the_environment_in_settings_only():
    for path in glob.glob(os.path.join(ROOT, "grappa_amd", "**", "*.py"), recursive=True):
        if os.path.basename(path) == "settings.py":
            continue
        with open(path, encoding="utf-8") as f:
            for no, line in enumerate(f, 1):
                if re.search(r"\benviron\b|getenv", line):
                    assert "WORLD_SIZE" in line or "MASTER_ADDR" in line, f"{path}:{no}: {line.strip()}"       # (torchrun's, not ours: dist.py)


def test_the_table_is_well_formed():
    names = [e.name for e in settings.TABLE]
    envs = [e.env for e in settings.TABLE if e.env]
    assert len(set(names)) == len(names) and len(set(envs)) == len(envs)
    for e in settings.TABLE:
        assert e.owner in ("backend", "ops", "writer", "host") and e.doc and (e.kind in ("flag", "int", "str") or callable(e.kind)), e.name
        assert e.env is None or re.fullmatch(r"GRAPPA_[A-Z_]+", e.env), e.name
    assert {e.name for e in settings.TABLE if e.env is None} == {"_tails", "plan_override", "splitk_reduce"}
    assert backend.DEFAULT_GEMM_PRECISION == "f32_f16x3"


# ---- defaults
def test_backend_defaults_are_those_of_the_hand_written_constructor(monkeypatch):
    be = _Cx(monkeypatch).be
    assert {e.name for e in settings.of("backend")} <= set(BACKEND_DEFAULTS) and len(BACKEND_DEFAULTS) == 27
    for name, want in BACKEND_DEFAULTS.items():
        assert _same(getattr(be, name), want), (name, getattr(be, name), want)


def test_ops_writer_and_host_defaults(monkeypatch):
    from grappa_amd import GrappaModel
    _Cx(monkeypatch)                                          # (clears GRAPPA_* from the environment)
    assert settings.read("FIRST_LAYER_ON_ATOM_ROWS") is True and settings.read("act_dtype") == "f32"
    if "GRAPPA_FIRST_LAYER_ROWS" not in os.environ and "GRAPPA_ACT_DTYPE" not in os.environ:
        assert ops.FIRST_LAYER_ON_ATOM_ROWS is True          # (read at import)
    pw = GrappaModel(**TINY).parameter_writer
    assert {e.name for e in settings.of("writer")} == set(WRITER_DEFAULTS)
    for name, want in WRITER_DEFAULTS.items():
        assert _same(getattr(pw, name), want), (name, getattr(pw, name), want)
    host = {e.name: settings.read(e.name) for e in settings.of("host")}
    assert host == dict(LIB_PATH=None, models_dir=None, trust_checkpoints=False, overlap=False, predict_graphs=True, host_plan=True)


# ---- the parse rule
@pytest.mark.parametrize("text, want", [("0", False), ("", False), ("1", True), ("no", True)])
def test_a_flag_is_false_for_0_and_the_empty_string_only(monkeypatch, text, want):
    cx = _Cx(monkeypatch)
    assert len(FLAGS) >= 20
    for e in FLAGS:
        monkeypatch.setenv(e.env, text)
        assert settings.read(e.name) is want, e.name
    be = backend.HipBackend()                                 # (over the recorder cx installed)
    for e in FLAGS:
        if e.owner == "backend":
            assert getattr(be, e.name) is want, e.name
    assert cx.be.defer_wgrads is True                         # the one built before: its values are its own


def test_the_odd_variables_parse_as_before(monkeypatch):
    _Cx(monkeypatch)
    monkeypatch.setenv("GRAPPA_GEMM_PRECISION_BWD", "")
    be = backend.HipBackend()
    assert be.gemm_precision_bwd_name is None and be.gemm_precision_bwd is None
    monkeypatch.setenv("GRAPPA_GEMM_PRECISION_BWD", "bf16x3")
    monkeypatch.setenv("GRAPPA_GEMM_PRECISION", "f32")
    monkeypatch.setenv("GRAPPA_WGRAD_QUEUE_GB", "0.5")
    monkeypatch.setenv("GRAPPA_PAIRS_MIN_ROWS", "100")
    be = backend.HipBackend()
    assert (be.gemm_precision_bwd_name, be.gemm_precision_bwd) == ("bf16x3", _lib.GEMM_PRECISIONS["bf16x3"])
    assert (be.gemm_precision_name, be.gemm_precision) == ("f32", _lib.GEMM_PRECISIONS["f32"])
    assert _same(be.wgrad_queue_bytes, 2 ** 29) and _same(be.pairs_min_rows, 100)
    monkeypatch.setenv("GRAPPA_GEMM_PRECISION", "fp64")
    with pytest.raises(ValueError):
        backend.HipBackend()
    monkeypatch.delenv("GRAPPA_GEMM_PRECISION")
    for text, want in ((None, (None, False)), ("", (None, False)), ("0", (False, True)), ("1", (True, True))):
        if text is not None:
            monkeypatch.setenv("GRAPPA_PLAN_TAILS", text)
        be = backend.HipBackend()
        assert (be._tails, be._tails_pinned) == want, text
        be.set_tail_launches(not want[0])                     # pinned: ignored
        assert be._tails is (want[0] if want[1] else True)
    for text, want in ((None, True), ("native", True), ("1", True), ("numpy", False), ("0", False), ("", False)):
        if text is not None:
            monkeypatch.setenv("GRAPPA_HOST_PLAN", text)
        assert settings.read("host_plan") is want, text


# ---- the stamp
def _trainer():
    from test_trainer import _items
    from grappa_amd import GrappaModel
    from grappa_amd.device_dataset import DeviceDataset
    from grappa_amd.trainer import Trainer
    torch.manual_seed(0)
    model = GrappaModel(**TINY)
    train = DeviceDataset(_items(list(range(300, 308))), device="cpu")
    return Trainer(model, train, None, batch_size=4, conf_strategy=4, lr=2e-3, start_qm_epochs=0, warmup_steps=2, energy_weight=1.0,
                   gradient_weight=0.8, param_weight=0.0, recorded=True)


def test_every_backend_setting_moves_the_stamp_and_both_stamps_made_of_it(monkeypatch, ref_backend):
    from grappa_amd.capture import CapturedForward
    tr = _trainer()                                           # (built on the test-only backend: the stub computes nothing)
    be = _Cx(monkeypatch).be
    monkeypatch.setattr(backend, "_BACKEND", be)
    fwd = CapturedForward.__new__(CapturedForward)            # (its constructor records on a GPU; the stamp needs these two only)
    fwd.be, fwd.model = be, tr.model
    stamps = lambda: (settings.launch_stamp(be), settings.launch_stamp(be, tr.model), fwd._config_stamp(), tr._step_stamp())      # noqa: E731
    base = stamps()
    assert len(base[0]) == len(settings.of("backend")) + len(settings.of("ops")) + len(settings.of("writer"))
    assert isinstance(base[2][-1], tuple) and base[2][-1] == tuple(p.data_ptr() for p in tr.model.parameters())
    for e in settings.of("backend"):
        old = getattr(be, e.name)
        setattr(be, e.name, _other(old))
        try:
            now = stamps()
            assert all(a != b for a, b in zip(now, base)), e.name
            hash(now)                                         # (the trainer keys a dict with it)
        finally:
            setattr(be, e.name, old)
        assert stamps() == base


def test_the_ops_and_writer_settings_move_the_stamp(monkeypatch, ref_backend):
    from grappa_amd.capture import CapturedForward
    tr = _trainer()
    be = _Cx(monkeypatch).be
    monkeypatch.setattr(backend, "_BACKEND", be)
    fwd = CapturedForward.__new__(CapturedForward)
    fwd.be, fwd.model = be, tr.model
    stamps = lambda: (settings.launch_stamp(be, tr.model), fwd._config_stamp(), tr._step_stamp())      # noqa: E731
    assert {e.name for e in settings.of("ops")} == {"act_dtype", "FIRST_LAYER_ON_ATOM_ROWS"}
    base = stamps()
    ops.set_activation_dtype("bf16")
    try:
        assert all(a != b for a, b in zip(stamps(), base))
    finally:
        ops.set_activation_dtype("f32")
    assert stamps() == base
    monkeypatch.setattr(ops, "FIRST_LAYER_ON_ATOM_ROWS", not ops.FIRST_LAYER_ON_ATOM_ROWS)
    assert all(a != b for a, b in zip(stamps(), base))
    monkeypatch.setattr(ops, "FIRST_LAYER_ON_ATOM_ROWS", not ops.FIRST_LAYER_ON_ATOM_ROWS)
    pw = tr.model.parameter_writer
    for e in settings.of("writer"):
        old = getattr(pw, e.name)
        setattr(pw, e.name, _other(old))
        try:
            assert all(a != b for a, b in zip(stamps(), base)), e.name
        finally:
            setattr(pw, e.name, old)
    assert stamps() == base


def test_the_stamp_of_a_backend_without_the_attributes(ref_backend):
    """the test-only backend has few of them: None stands in, nothing raises"""
    stamp = settings.launch_stamp(ref_backend)
    assert len(stamp) == len(settings.of("backend")) + len(settings.of("ops")) + len(settings.of("writer")) and None in stamp
    tr = _trainer()
    assert tr._step_stamp()[-len(stamp):] == settings.launch_stamp(ref_backend, tr.model)


def test_a_recorded_step_is_stored_under_the_step_key(monkeypatch, ref_backend):
    """`train_step_recorded` with the GPU's part replaced: the key it files the step under is `_step_key` of the batch"""
    from grappa_amd import capture

    class Stream:
        def wait_event(self, ev):
            pass

    class Event:
        def record(self, stream=None):
            pass

    class Step:
        def __init__(self, *a, **k):
            pass

        def __call__(self):
            return torch.zeros(())

    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: Stream())
    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(capture, "CapturedTrainStep", Step)
    tr = _trainer()
    ids = np.arange(4)
    g, names = tr.train_set.collate(ids, tr.conf_strategy)
    tr.train_step_recorded(ids, prepared=(g, names, Event(), {"n1": 1}, {"n1": 1}))
    assert tr.recorded_stats["graphs_recorded"] == 1 and list(tr._steps) == [tr._step_key(g)]
    key = tr._step_key(g)
    assert len(key) == 3 and key[0] == capture.train_signature(g) and key[1] == tr._step_stamp() and key[2] is None
