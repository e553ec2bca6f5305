"""The call skeleton under the C++ host classes (flan_amd/host/device_call.h), driven by tests/cpp/device_call_test.cpp: a stand-alone
program over the header alone, with recording stand-ins for the few symbols it references -- no device, neither library.  On the log of
events: the success path synchronises exactly once, before the workspace and the arguments go back to the cache, and hands the output
block over; a failure before any launch synchronises nothing and releases what was acquired; a failure or an exception after a launch
synchronises once before the first release; a failing synchronise gives a null result and one reported line."""
import host_cpp


def test_blocks_go_back_only_after_the_synchronise():
    host_cpp.build("device_call_test", host_library=False)
    host_cpp.run("device_call_test", timeout=60)
