"""CPU checks of the device-resident learning loop's boundary (abnn.h
abnn_engine_*): the ctypes mirrors match the C layouts, the default config is
abnn::EngineConfig's, and a null handle is refused without a GPU."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_engine_struct_layouts_match_c(tmp_path):
    from abnn_amd import _lib

    prog = tmp_path / "sz.c"
    prog.write_text('#include "abnn/abnn.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(abnn_engine_config),'
                    'sizeof(abnn_engine_state), offsetof(abnn_engine_config, filter_tau),'
                    'offsetof(abnn_engine_config, teacher_seed), offsetof(abnn_engine_state, teach),'
                    'offsetof(abnn_engine_state, last_loss));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_lib.EngineConfig), C.sizeof(_lib.EngineState), _lib.EngineConfig.filter_tau.offset,
            _lib.EngineConfig.teacher_seed.offset, _lib.EngineState.teach.offset, _lib.EngineState.last_loss.offset]
    assert got == want
    assert got[:2] == [64, 48]


def test_default_engine_config_equals_engine_hpp(tmp_path):
    """abnn_default_engine_config against abnn::EngineConfig's member
    initialisers, printed by a C++ snippet that includes only engine.hpp."""
    import abnn_amd

    prog = tmp_path / "cfg.cpp"
    prog.write_text('#include <abnn/engine.hpp>\n#include <cstdio>\n'
                    'int main(){abnn::EngineConfig c;std::printf("%.9g %.9g %.17g %d %zu %.17g %.9g %.9g %zu %.17g %llu\\n",'
                    'c.input_rate_hz,c.peak_decay,c.filter_tau,(int)c.use_fir,c.fir_size,c.dt_sec,c.rate_alpha,'
                    'c.max_observed,c.win_size,c.last_loss,(unsigned long long)c.teacher_seed);return 0;}\n')
    exe = tmp_path / "cfg"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    hpp = [float(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    c = abnn_amd.default_engine_config()
    got = [c.input_rate_hz, c.peak_decay, c.filter_tau, c.use_fir, c.fir_size, c.dt_sec, c.rate_alpha,
           c.max_observed, c.win_size, c.last_loss, c.teacher_seed]
    f32 = lambda x: C.c_float(x).value
    assert got == [1000, f32(0.999), 0.02, True, 20, 0.0009, 0.5, 0.5, 1000, 0.25, 1]
    assert got == [f32(hpp[0]), f32(hpp[1]), *hpp[2:6], f32(hpp[6]), f32(hpp[7]), *hpp[8:]]
    assert c.trace_passes == 4096


def test_engine_null_arguments_are_invalid_without_a_gpu():
    from abnn_amd import _lib

    lib = _lib.load()
    cfg = _lib.EngineConfig()
    lib.abnn_default_engine_config(C.byref(cfg))
    out = C.c_void_p()
    assert lib.abnn_engine_create(None, C.byref(cfg), C.byref(out)) == 1  # ABNN_ERR_INVALID
    assert not out.value
    st = _lib.EngineState()
    assert lib.abnn_engine_destroy(None) == 1
    assert lib.abnn_engine_run(None, None, None, 1, None) == 1
    assert lib.abnn_engine_get_state(None, C.byref(st)) == 1
    assert lib.abnn_engine_get_rates(None, None, None, None, 0) == 1
    assert lib.abnn_engine_read_trace(None, 0, 0, None, None) == 1
