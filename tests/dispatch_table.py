"""What the int8 GEMM dispatcher answers through the C-ABI's query functions, over a grid of shapes -- shared by tests/test_dispatch_table_cpu.py
and tests/golden/make_golden_dispatch.py.  The library reads its switches once per process, so every environment gets a child process of its own
(`python tests/dispatch_table.py LIB` prints the rows as JSON); the children only call query functions and need no GPU."""
import ctypes
import json
import os
import subprocess
import sys

MS = (1, 4, 16, 17, 32, 33, 48, 64, 65, 96, 128, 129, 160, 161, 192, 256, 257, 320, 384, 512, 640, 768, 1024, 1025, 1280, 1536, 2000, 2048, 2304, 3072, 4096,
      8192, 16384, 65536)
NKS = ((4096, 4096), (11008, 4096), (4096, 11008), (12288, 4096), (5120, 5120), (20480, 5120), (5120, 20480), (14336, 4096), (4096, 14336), (1024, 4096),
       (13312, 4096), (12284, 4096), (4095, 4096), (4096, 4095), (4096, 128), (4096, 256), (8192, 8192), (4098, 4096), (256, 16384), (128, 128))
# "" = the default environment; the others are the switches tests and tools force
ENVS = ("", "ASQ_NO_TAIL=1", "ASQ_SPLITK_FIX=0", "ASQ_SK_IMPL=1", "ASQ_GEMM_KERNEL=p8q ASQ_KSPLIT=3", "ASQ_GEMM_KERNEL=p8 ASQ_KSPLIT=3")
SWITCHES = ("ASQ_NO_TAIL", "ASQ_SPLITK_FIX", "ASQ_SK_IMPL", "ASQ_GEMM_KERNEL", "ASQ_KSPLIT", "ASQ_MMA", "ASQ_OFFSETS", "ASQ_FUSED_FORWARD", "ASQ_SK_NT",
            "ASQ_WS_GRID", "ASQ_WS_NT", "ASQ_P16_PERSIST")
COLUMNS = ("M", "N", "K", "kernel_name", "gemm_workspace_bytes", "linear_w8a8_workspace_bytes", "offsets_supported[f32,f16,bf16]",
           "forward_fused_supported[f16; round,div,per_token]")


def rows(lib_path):
    """The table of the library at lib_path under THIS process's environment."""
    h = ctypes.CDLL(lib_path)
    i64, sz = ctypes.c_int64, ctypes.c_size_t
    h.asq_gemm_kernel_name.restype, h.asq_gemm_kernel_name.argtypes = ctypes.c_char_p, [i64, i64, i64]
    h.asq_gemm_workspace_bytes.restype, h.asq_gemm_workspace_bytes.argtypes = sz, [i64, i64, i64]
    h.asq_linear_w8a8_workspace_bytes.restype, h.asq_linear_w8a8_workspace_bytes.argtypes = sz, [i64, i64, i64]
    h.asq_offsets_supported.restype, h.asq_offsets_supported.argtypes = ctypes.c_int, [i64, i64, i64, ctypes.c_int]
    h.asq_forward_fused_supported.restype, h.asq_forward_fused_supported.argtypes = ctypes.c_int, [i64, i64, i64, ctypes.c_int, ctypes.c_int]
    out = []
    for (N, K) in NKS:
        for M in MS:
            out.append([M, N, K, h.asq_gemm_kernel_name(M, N, K).decode(), h.asq_gemm_workspace_bytes(M, N, K), h.asq_linear_w8a8_workspace_bytes(M, N, K),
                        [h.asq_offsets_supported(M, N, K, dt) for dt in (0, 1, 2)], [h.asq_forward_fused_supported(M, N, K, 1, mode) for mode in (0, 1, 2)]])
    return out


def rows_in_child(lib_path, env):
    """The table under `env` ("KEY=VAL KEY=VAL"), from a fresh process."""
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(kv.split("=", 1) for kv in env.split())
    r = subprocess.run([sys.executable, os.path.abspath(__file__), lib_path], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


if __name__ == "__main__":
    json.dump(rows(sys.argv[1]), sys.stdout)
