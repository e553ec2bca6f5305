// flan/AudioMod.h -- the modification callback of the granular methods (mirrors the reference's src/flan/Audio/AudioMod.h:10-49 and
// AudioMod.cpp): a callable void( T &, Second ) with the execution policy the user allows for it, or nothing at all (is_null()).
// Move-only, like the reference's.
#pragma once
#include <functional>
#include <type_traits>
#include <utility>

#include "flan/defines.h"

namespace flan {

template<typename T>
class SoundMod
	{
public:
	using FuncType = std::function<void( T &, Second )>;

	SoundMod( const SoundMod & ) = delete;
	SoundMod & operator=( const SoundMod & ) = delete;
	SoundMod( SoundMod && ) = default;
	SoundMod & operator=( SoundMod && ) = delete;                                // (the reference defaults it; its const member deletes it all the same)
	~SoundMod() = default;

	template<typename C, std::enable_if_t<std::is_convertible_v<C, FuncType> && !std::is_same_v<std::decay_t<C>, std::nullptr_t>
		&& !std::is_same_v<std::decay_t<C>, SoundMod>, int> = 0>
	SoundMod( C f_, ExecutionPolicy policy_ = ExecutionPolicy::Parallel_Unsequenced ) : func( std::move( f_ ) ), policy( policy_ ), null( false ) {}
	SoundMod() : func( nullptr ), policy( ExecutionPolicy::Parallel_Unsequenced ), null( true ) {}                  // AudioMod.cpp:8-13

	void operator()( T & in, Second t ) const { if( null ) return; func( in, t ); }                                // :16-20
	bool is_null() const { return null; }
	ExecutionPolicy get_execution_policy() const { return policy; }

private:
	FuncType func;
	ExecutionPolicy policy;
	const bool null;
	};

class Audio;
using AudioMod = SoundMod<Audio>;
class PV;
using PVMod = SoundMod<PV>;

} // namespace flan
