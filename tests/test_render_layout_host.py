"""The output layout of a render call (csrc/render_layout.h, the one owner of which outputs exist and where they lie in the pools)
walked on the host under sanitizers: tests/native/render_layout_test.cpp."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_on_the_host_under_sanitizers(tmp_path):
    """Over level sets x ndc x per-sample masks x predict_visibility x secondary views x given fine depths x keep_activations x
    sample counts: the slots tile each pool exactly, presence and ``returned`` follow the rules spelled out in the program, bound
    pointers stay inside the pools; two hand-derived layouts are pinned.  And the backward workspace (backward_regions) over ray
    counts x sample counts x admitted level sets x inner sizes around the 64-float rounding, in order and side by side: totals equal
    the formulas, regions are disjoint and in level order, the in-order layout fits the side-by-side allocation.  AddressSanitizer +
    UBSan, no GPU."""
    exe = str(tmp_path / 'render_layout_test')
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        '-I', os.path.join(REPO, 'include'), os.path.join(REPO, 'tests', 'native', 'render_layout_test.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'))
    assert r.returncode == 0 and 'render_layout_test: OK' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
