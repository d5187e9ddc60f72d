// handles.h -- the opaque handle types of include/eesen_hip.h as the library sees them.
#pragma once
#include "net.h"

struct eesen_net : public eesen::Net { using eesen::Net::Net; };
struct eesen_ctc : public eesen::Ctc { using eesen::Ctc::Ctc; };
struct eesen_ce : public eesen::CeLoss { using eesen::CeLoss::CeLoss; };
struct eesen_lm : public eesen::TokenLm {};
struct eesen_lex : public eesen::Lexicon {};
