# The program of the flow composition tests (tests/test_compose_host.py):
#   make -C tests/cpp -f compose.mk args_compose
ROOT := $(abspath ../..)
CSRC := $(ROOT)/optical-flow-using-dense-inverse-search_amd/csrc

# The aliasing rule with an output that may be an input itself, and the points
# extent (csrc/dis_args.h), under ASan + UBSan, any finding aborts: compiled and
# run (args_compose_host.cpp has its own main).
SAN := -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -g -O1
ARGS_OUT ?= args_compose_host
args_compose: args_compose_host.cpp far_cases.h $(CSRC)/dis_args.h
	g++ $(SAN) -std=c++17 -Wall -I$(CSRC) args_compose_host.cpp -o $(ARGS_OUT)
	ASAN_OPTIONS=detect_leaks=0 $(abspath $(ARGS_OUT))

clean:
	rm -f args_compose_host
