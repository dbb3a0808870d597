# The program of the flow fill tests (tests/test_fill_host.py):
#   make -C tests/cpp -f fill.mk args_fill
ROOT := $(abspath ../..)
CSRC := $(ROOT)/optical-flow-using-dense-inverse-search_amd/csrc

# The levels, the workspace size, the grid limit and the aliasing rule of
# dis_flow_fill (csrc/dis_args.h), under ASan + UBSan, any finding aborts:
# compiled and run (args_fill_host.cpp has its own main).
SAN := -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1
ARGS_OUT ?= args_fill_host
args_fill: args_fill_host.cpp far_cases.h $(CSRC)/dis_args.h
	g++ $(SAN) -std=c++17 -Wall -I$(CSRC) args_fill_host.cpp -o $(ARGS_OUT)
	ASAN_OPTIONS=detect_leaks=0 $(abspath $(ARGS_OUT))

clean:
	rm -f args_fill_host
