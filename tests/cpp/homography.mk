# The programs of the homography tests (tests/test_homography_host.py,
# tests/test_gpu_homography.py):
#   make -C tests/cpp -f homography.mk args_homography
#   make -C tests/cpp -f homography.mk test_homography
ROOT := $(abspath ../..)
PKG := $(ROOT)/optical-flow-using-dense-inverse-search_amd/disflow
CSRC := $(ROOT)/optical-flow-using-dense-inverse-search_amd/csrc

# dis_homography_stabilize (csrc/dis_stabilize.cpp, plain C++) and the argument
# rules of the homography family (csrc/dis_args.h), under ASan + UBSan, any
# finding aborts: compiled and run (args_homography_host.cpp has its own main).
SAN := -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1
ARGS_OUT ?= args_homography_host
args_homography: args_homography_host.cpp far_cases.h $(CSRC)/dis_stabilize.cpp $(CSRC)/dis_args.h $(ROOT)/include/dis_abi.h
	g++ $(SAN) -std=c++17 -Wall -ffp-contract=off -I$(ROOT)/include -I$(CSRC) args_homography_host.cpp \
	    $(CSRC)/dis_stabilize.cpp -o $(ARGS_OUT)
	ASAN_OPTIONS=detect_leaks=0 $(abspath $(ARGS_OUT))

# The facade's homography entries against the library (a GPU test runs it).
HOMOGRAPHY_OUT ?= test_homography
test_homography: test_homography.cpp $(ROOT)/include/dis/dis.hpp $(ROOT)/include/dis_abi.h
	g++ -std=c++17 -O2 -Wall -I$(ROOT)/include test_homography.cpp -o $(HOMOGRAPHY_OUT) -L$(PKG) -ldis_hip \
	    -Wl,-rpath,$(PKG) -Wl,-rpath,/opt/rocm/lib

clean:
	rm -f args_homography_host test_homography
