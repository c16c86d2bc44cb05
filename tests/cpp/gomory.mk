# The host side of relp_gomory_cuts (rust-lp_amd/csrc/relp_gomory.hpp over relp_layout.cpp, plain C++17): plain g++, no library,
# no GPU.  `make -C tests/cpp -f gomory.mk`
#   test_gomory       the argument checks, the statuses decided per entry, the slack rows of a Layout, the beta chain
#   test_gomory_asan  the same program with -fsanitize=address,undefined (a stand-alone program: no preload)
CXX ?= g++
ROOT := ../..
CSRC := $(ROOT)/rust-lp_amd/csrc
DEPS := test_gomory.cpp $(CSRC)/relp_gomory.hpp $(CSRC)/relp_layout.cpp $(CSRC)/relp_layout.hpp $(ROOT)/include/relp_engine.h

all: test_gomory test_gomory_asan

test_gomory: $(DEPS)
	$(CXX) -std=c++17 -O1 -Wall -Wextra -I$(CSRC) test_gomory.cpp $(CSRC)/relp_layout.cpp -o $@

test_gomory_asan: $(DEPS)
	$(CXX) -std=c++17 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) test_gomory.cpp $(CSRC)/relp_layout.cpp -o $@

clean:
	rm -f test_gomory test_gomory_asan
