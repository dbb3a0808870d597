# The programs of the stabilisation tests (tests/test_stabilize_host.py,
# tests/test_gpu_stabilize.py):
#   make -C tests/cpp -f stabilize.mk args_stabilize
#   make -C tests/cpp -f stabilize.mk test_stabilize
ROOT := $(abspath ../..)
PKG := $(ROOT)/optical-flow-using-dense-inverse-search_amd/disflow
CSRC := $(ROOT)/optical-flow-using-dense-inverse-search_amd/csrc

# dis_motion_stabilize (csrc/dis_stabilize.cpp, plain C++) and the argument rules
# of it and of dis_warp_motion_u8 (csrc/dis_args.h), under ASan + UBSan, any
# finding aborts: compiled and run (args_stabilize_host.cpp has its own main).
SAN := -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1
ARGS_OUT ?= args_stabilize_host
args_stabilize: args_stabilize_host.cpp far_cases.h $(CSRC)/dis_stabilize.cpp $(CSRC)/dis_args.h $(ROOT)/include/dis_abi.h
	g++ $(SAN) -std=c++17 -Wall -ffp-contract=off -I$(ROOT)/include -I$(CSRC) args_stabilize_host.cpp \
	    $(CSRC)/dis_stabilize.cpp -o $(ARGS_OUT)
	ASAN_OPTIONS=detect_leaks=0 $(abspath $(ARGS_OUT))

# The facade's stabilisation entries against the library (a GPU test runs it).
STAB_OUT ?= test_stabilize
test_stabilize: test_stabilize.cpp $(ROOT)/include/dis/dis.hpp $(ROOT)/include/dis_abi.h
	g++ -std=c++17 -O2 -Wall -I$(ROOT)/include test_stabilize.cpp -o $(STAB_OUT) -L$(PKG) -ldis_hip \
	    -Wl,-rpath,$(PKG) -Wl,-rpath,/opt/rocm/lib

clean:
	rm -f args_stabilize_host test_stabilize
