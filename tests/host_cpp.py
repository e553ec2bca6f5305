"""Building and running the stand-alone C++ drivers of tests/cpp/: one plain helper for the test_*_host_cpp.py modules (imported like the
*_reference.py modules; no fixture).  A driver is tests/cpp/<name>.cpp over libflan_host.so + libflanhip.so, compiled to tests/cpp/<name>
when that is older than its source or the host library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "flan_amd")


def binary(name):
    return os.path.join(ROOT, "tests", "cpp", name)


def build(name, fp_contract_off=True, host_library=True, flags=()):
    """host_library=False: a program that stands alone over flan_amd/host's private headers and links neither library"""
    src, out = binary(name) + ".cpp", binary(name)
    deps, link = [src], []
    if host_library:
        subprocess.run(["make", "-s", "-C", os.path.join(LIBDIR, "host")], check=True)
        deps.append(os.path.join(LIBDIR, "libflan_host.so"))
        link = ["-L" + LIBDIR, "-lflan_host", "-lflanhip", "-Wl,-rpath," + LIBDIR]
    else:
        deps += [os.path.join(LIBDIR, "host", h) for h in ("device_call.h", "device_block.h")]
        flags = ["-I" + os.path.join(LIBDIR, "host")] + list(flags)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17"] + (["-ffp-contract=off"] if fp_contract_off else []) + list(flags)
                       + ["-I" + os.path.join(ROOT, "include"), src, "-o", out] + link + ["-lpthread"], check=True)
    return out


def run(name, *args, check=True, timeout=600):
    """check: the output is printed and the driver must exit 0 and say PASSED; the completed process either way"""
    env = dict(os.environ, LD_LIBRARY_PATH=LIBDIR + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([binary(name)] + list(args), capture_output=True, text=True, env=env, timeout=timeout)
    if check:
        print(r.stdout, r.stderr)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "PASSED" in r.stdout
    return r


def driver(name, check=True, timeout=600, **build_options):
    """( BIN, _build(), _run( *args ) ) of one driver, as the test modules name them"""
    return (binary(name), lambda: build(name, **build_options),
            lambda *args, timeout=timeout: run(name, *args, check=check, timeout=timeout))
