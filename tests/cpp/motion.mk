# The program of the global-motion tests (tests/test_motion_host.py):
#   make -C tests/cpp -f motion.mk args_motion
ROOT := $(abspath ../..)
CSRC := $(ROOT)/optical-flow-using-dense-inverse-search_amd/csrc

# The chunk count, the workspace size, the grid limits and the overlap rule of
# dis_flow_fit_motion (csrc/dis_args.h), under ASan + UBSan, any finding aborts:
# compiled and run (args_motion_host.cpp has its own main).
SAN := -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1
ARGS_OUT ?= args_motion_host
args_motion: args_motion_host.cpp far_cases.h $(CSRC)/dis_args.h
	g++ $(SAN) -std=c++17 -Wall -I$(CSRC) args_motion_host.cpp -o $(ARGS_OUT)
	ASAN_OPTIONS=detect_leaks=0 $(abspath $(ARGS_OUT))

clean:
	rm -f args_motion_host
