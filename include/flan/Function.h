// flan/Function.h -- the callback type of the PV frame processors (mirrors the reference's src/flan/Function.h:35-265 and
// FunctionSample.h:18-199 for the parts the phase-vocoder path uses).
//
// A Function<I,O> is either a constant O or a std::function<O(I)>, plus the execution policy the user allows for
// evaluating it.  Device kernels cannot call back into host code, so the PV methods sample a Function on the host over the
// (frame, bin) grid (Function.h:155-171) and upload the grid; a CONSTANT never touches the host (the grid is filled on the
// device).  Note a reference quirk we do not reproduce: there a constant Function breaks stretch/repitch (the in-place
// prefix sum doubles the single shared constant each step, FunctionSample.h:186-190 with PVModify.cpp:278-280,376-378);
// here a constant c behaves exactly like the callable `[](TF){ return c; }`.
#pragma once
#include <algorithm>
#include <cmath>
#include <functional>
#include <thread>
#include <new>
#include <type_traits>
#include <utility>
#include <variant>
#include <vector>

#include "flan/defines.h"

namespace flan {

namespace detail {
// the host runtime in libflan_host (flan_amd/host/host_runtime.cpp): a persistent worker pool and page-locked staging memory
int host_workers();                                                            // threads a parallel region runs on
void pool_run( int n_tasks, void ( *fn )( void *, int ), void * ctx );         // fn( ctx, i ) for i in [0, n_tasks), load balanced
void * staging_acquire( size_t bytes );                                        // page-locked when large and a device is there
void staging_release( void * p ) noexcept;

// Parallel policies: split the index range over the host cores in contiguous grains; sequential policies: a plain loop.
template<typename F>
void for_each_index( int begin, int end, ExecutionPolicy policy, const F & body, int min_parallel = 128 )
	{
	const int n = end - begin;
	const bool parallel = policy == ExecutionPolicy::Parallel_Sequenced || policy == ExecutionPolicy::Parallel_Unsequenced;
	if( !parallel || n < min_parallel ) { for( int i = begin; i < end; ++i ) body( i ); return; }
	struct Job { const F * body; int begin, end, grain; } job{ &body, begin, end, std::max( 1, n / ( host_workers() * 8 ) ) };
	pool_run( ( n + job.grain - 1 ) / job.grain, []( void * ctx, int task )
		{
		const Job & j = *static_cast<const Job*>( ctx );
		const int lo = j.begin + task * j.grain, hi = std::min( j.end, lo + j.grain );
		for( int i = lo; i < hi; ++i ) ( *j.body )( i );
		}, &job );
	}

// Allocator of the sampled grids: staging memory, and no zero fill for the value-initialised elements a sample overwrites anyway
template<typename T>
struct StagingAllocator
	{
	using value_type = T;
	StagingAllocator() = default;
	template<typename U> StagingAllocator( const StagingAllocator<U> & ) {}
	T * allocate( size_t n ) { return static_cast<T*>( staging_acquire( n * sizeof( T ) ) ); }
	void deallocate( T * p, size_t ) noexcept { staging_release( p ); }
	template<typename U, typename... Args> void construct( U * p, Args &&... args )
		{
		if constexpr( sizeof...( args ) == 0 && std::is_trivially_default_constructible_v<U> ) (void) p;
		else ::new( static_cast<void*>( p ) ) U( std::forward<Args>( args )... );
		}
	template<typename U> bool operator==( const StagingAllocator<U> & ) const { return true; }
	template<typename U> bool operator!=( const StagingAllocator<U> & ) const { return false; }
	};
template<typename T> using StagingVector = std::vector<T, StagingAllocator<T>>;
}

// FunctionSample.h:173-199: a sampled function, either one constant or a grid [big][small]
template<typename O>
struct FunctionSample2d
	{
	using Vector = detail::StagingVector<O>;                                      // a std::vector in everything but where its memory comes from
	std::variant<O, Vector> value;
	size_t count;
	size_t small_dim_size;
	bool is_constant() const { return std::holds_alternative<O>( value ); }
	const O & get_constant() const { return std::get<O>( value ); }
	Vector & get_vector() { return std::get<Vector>( value ); }
	const Vector & get_vector() const { return std::get<Vector>( value ); }
	size_t size() const { return count; }
	O at( Frame f, Bin b ) const { return is_constant() ? get_constant() : get_vector()[size_t( f ) * small_dim_size + b]; }
	};

template<typename I, typename O>
struct Function
	{
	using StdFuncType = std::function<O( I )>;
	using ReturnType = O;
	using ArgType = I;

	Function( const Function & ) = delete;
	Function & operator=( const Function & ) = delete;
	Function( Function && ) = default;
	Function & operator=( Function && ) = default;

	template<typename T, std::enable_if_t<std::is_convertible_v<T, O> && !std::is_convertible_v<T, StdFuncType>, int> = 0>
	Function( T t0 ) : f( static_cast<O>( t0 ) ), execution_policy( ExecutionPolicy::Parallel_Unsequenced ) {}

	template<typename T, std::enable_if_t<std::is_convertible_v<T, StdFuncType>, int> = 0>
	Function( T && f_, ExecutionPolicy policy = ExecutionPolicy::Parallel_Unsequenced )
		: f( StdFuncType( std::forward<T>( f_ ) ) ), execution_policy( policy ) {}

	Function copy() const
		{
		if( is_constant() ) return Function( std::get<O>( f ) );
		return Function( std::get<StdFuncType>( f ), execution_policy );
		}
	bool is_constant() const { return std::holds_alternative<O>( f ); }
	const O & get_constant() const { return std::get<O>( f ); }
	ExecutionPolicy get_execution_policy() const { return execution_policy; }

	// (an O that cannot be copied -- Function<Second, Audio>, the grain source of Audio::synthesize_grains -- can only come from a callable)
	O operator()( I t ) const
		{
		if constexpr( std::is_copy_constructible_v<O> ) { if( is_constant() ) return std::get<O>( f ); }
		return std::get<StdFuncType>( f )( t );
		}

	// Function.h:155-171: sample on the grid x in [x_start, x_end), y in [y_start, y_end), argument ( x*x_scale, y*y_scale ),
	// result laid out [x][y].  Only for I constructible from two floats (TF).
	FunctionSample2d<O> sample( float x_start, float x_end, float x_scale, float y_start, float y_end, float y_scale ) const
		{
		const int x_size = int( std::ceil( x_end - x_start ) );
		const int y_size = int( std::ceil( y_end - y_start ) );
		if( is_constant() ) return FunctionSample2d<O>{ std::get<O>( f ), size_t( x_size ) * y_size, size_t( y_size ) };
		typename FunctionSample2d<O>::Vector out( size_t( x_size ) * y_size );
		// (the grid's memory is not cleared: whole-number bounds -- every call of the PV methods -- write every slot; fractional ones leave slots
		// the reference's value-initialised vector holds as O())
		if( x_start != std::floor( x_start ) || x_end != std::floor( x_end ) || y_start != std::floor( y_start ) || y_end != std::floor( y_end ) )
			std::fill( out.begin(), out.end(), O() );
		sample_into( out.data(), x_start, x_end, x_scale, y_start, y_end, y_scale );
		return FunctionSample2d<O>{ std::move( out ), size_t( x_size ) * y_size, size_t( y_size ) };
		}

	// the same grid written to memory of the caller's (rows [x_start, x_end) only, row x at out + (x - x_start) * y_size): what
	// lets the PV methods upload one part of a grid while the next is being sampled.  Not for constants.
	void sample_into( O * out, float x_start, float x_end, float x_scale, float y_start, float y_end, float y_scale ) const
		{
		const int y_size = int( std::ceil( y_end - y_start ) );
		const StdFuncType & fn = std::get<StdFuncType>( f );
		// The reference's own arithmetic (Function.h:163-168), which matters when a bound has a fractional part: x runs over the INTEGERS
		// [ int( x_start ), int( x_end ) ) (iota_iter takes an int), y from int( y_start ) while y < y_end (an int against a float), and a point's
		// slot is buffer_access( int( y - y_start ), int( x - x_start ), y_size ) -- the float differences truncated, so with fractional
		// starts two neighbouring points can share a slot (the later one stays) and slots past int( x_end ) keep their initial value.
		// Pinned by tests/golden/ref_made/function_sample.npz, made by the reference's header itself.
		detail::for_each_index( int( x_start ), int( x_end ), execution_policy, [&]( int x )
			{
			const int row = int( float( x ) - x_start );                             // (0 for the first x whatever the fraction: |int( s ) - s| < 1)
			for( int y = int( y_start ); y < y_end; ++y )
				out[size_t( row ) * y_size + int( float( y ) - y_start )] = fn( I{ x * x_scale, y * y_scale } );
			}, 16 );
		}

	// Function.h:141-153: sample a function of one variable at x*scale, x in [start, end); a constant stays a constant
	// (FunctionSample.h:18-40)
	struct Sample1d
		{
		std::variant<O, std::vector<O>> value;
		bool is_constant() const { return std::holds_alternative<O>( value ); }
		const O & get_constant() const { return std::get<O>( value ); }
		const std::vector<O> & get_vector() const { return std::get<std::vector<O>>( value ); }
		};
	Sample1d sample( int start, int end, float scale ) const
		{
		if( is_constant() ) return Sample1d{ std::get<O>( f ) };
		std::vector<O> out( size_t( std::max( end - start, 0 ) ) );
		const StdFuncType & fn = std::get<StdFuncType>( f );
		detail::for_each_index( start, end, execution_policy, [&]( int x ){ out[size_t( x - start )] = fn( I( x * scale ) ); } );
		return Sample1d{ std::move( out ) };
		}

private:
	std::variant<O, StdFuncType> f;
	ExecutionPolicy execution_policy;
	};

// Utility/Interpolator.h: a [0,1] -> [0,1] shaping function used when a frame (bin) pair is spread over the output.
// The NAMED interpolators (Utility/Interpolator.cpp:14-101) carry a kind the device kernels can evaluate themselves
// (FLANHIP_INTERP_* in flanhip.h); an interpolator built from an arbitrary callable has kind -1 and only runs in the
// methods that sample it on the host first (time_extrapolate).  modify_time / modify_frequency / stretch / repitch run
// Interpolator::linear(), the reference's default, only.
class Interpolator
	{
public:
	static Interpolator linear()       { return Interpolator( 0, []( float x ){ return x; } ); }
	static Interpolator midpoint()     { return Interpolator( 1, []( float ){ return 0.5f; } ); }
	static Interpolator nearest()      { return Interpolator( 2, []( float x ){ return std::round( x ); } ); }
	static Interpolator floor()        { return Interpolator( 3, []( float ){ return 0.0f; } ); }
	static Interpolator ceil()         { return Interpolator( 4, []( float ){ return 1.0f; } ); }
	static Interpolator smoothstep()   { return Interpolator( 5, []( float x ){ return x * x * ( 3.0f - 2.0f * x ); } ); }
	static Interpolator smootherstep() { return Interpolator( 6, []( float x ){ return x * x * x * ( x * ( x * 6.0f - 15.0f ) + 10.0f ); } ); }
	static Interpolator sqrt()         { return Interpolator( 7, []( float x ){ return std::sqrt( x ); } ); }
	static Interpolator sine()         { return Interpolator( 8, []( float x ){ return ( 1.0f - std::cos( std::acos( -1.0f ) * x ) ) / 2.0f; } ); }
	template<typename T, std::enable_if_t<std::is_convertible_v<T, std::function<float( float )>>, int> = 0>
	Interpolator( T && fn ) : kind_( -1 ), f_( std::forward<T>( fn ) ) {}
	float operator()( float x ) const { return f_( x ); }
	bool is_linear() const { return kind_ == 0; }
	int kind() const { return kind_; }                                            // FLANHIP_INTERP_*, or -1
private:
	Interpolator( int kind, std::function<float( float )> fn ) : kind_( kind ), f_( std::move( fn ) ) {}
	int kind_;
	std::function<float( float )> f_;
	};

// The reference's waveforms::sine / square / saw / triangle (Function.cpp:32-39) are plain std::functions whose identity is lost once they are
// inside a Function.  Here a Waveform carries a kind the device can evaluate (FLANHIP_WAVEFORM_* in flanhip.h), as an Interpolator does; one
// built from a callable has kind -1 and is evaluated on the host under its policy.  Each named one is fmod( t, 1.0f ), which keeps the sign
// of t, followed by the reference's expression.
class Waveform
	{
public:
	static Waveform sine()     { return Waveform( 0, []( Second t ){ const Second t0 = std::fmod( t, 1.0f ); return std::sin( pi2 * t0 ); } ); }
	static Waveform square()   { return Waveform( 1, []( Second t ){ const Second t0 = std::fmod( t, 1.0f ); return t0 < 0.5f ? -1.0f : 1.0f; } ); }
	static Waveform saw()      { return Waveform( 2, []( Second t ){ const Second t0 = std::fmod( t, 1.0f ); return -1.0f + 2.0f * t0; } ); }
	static Waveform triangle() { return Waveform( 3, []( Second t ){ const Second t0 = std::fmod( t, 1.0f ); return t0 < 0.5f ? -1.0f + 4.0f * t0 : 3.0f - 4.0f * t0; } ); }
	template<typename T, std::enable_if_t<std::is_convertible_v<T, std::function<Amplitude( Second )>> && !std::is_same_v<std::decay_t<T>, Waveform>, int> = 0>
	Waveform( T && fn, ExecutionPolicy policy = ExecutionPolicy::Parallel_Unsequenced ) : kind_( -1 ), f_( std::forward<T>( fn ) ), policy_( policy ) {}
	Amplitude operator()( Second t ) const { return f_( t ); }
	int kind() const { return kind_; }                                            // FLANHIP_WAVEFORM_*, or -1
	ExecutionPolicy get_execution_policy() const { return policy_; }
private:
	Waveform( int kind, std::function<Amplitude( Second )> fn ) : kind_( kind ), f_( std::move( fn ) ), policy_( ExecutionPolicy::Parallel_Unsequenced ) {}
	int kind_;
	std::function<Amplitude( Second )> f_;
	ExecutionPolicy policy_;
	};

namespace waveforms {
inline const Waveform sine = Waveform::sine();
inline const Waveform square = Waveform::square();
inline const Waveform saw = Waveform::saw();
inline const Waveform triangle = Waveform::triangle();
}

/** The envelope of Function.cpp:11-30: 0 outside [0, a + d + s + r]; ( t / a )^aExp while attacking; ( 1 - ( t - a ) / d )^dExp * ( 1 - sLvl ) + sLvl
 *  while decaying; sLvl while sustaining; ( 1 - ( t - a - d - s ) / r )^rExp * sLvl while releasing; 0 at t == a + d + s + r exactly.  Every
 *  operation in fp32, in that order. */
inline Function<Second, Amplitude> ADSR( Second a, Second d, Second s, Second r, Amplitude sLvl, float aExp = 1, float dExp = 1, float rExp = 1 )
	{
	return Function<Second, Amplitude>( [a, d, s, r, sLvl, aExp, dExp, rExp]( Second t ) -> Amplitude
		{
		if( t < 0 || t > a + d + s + r ) return 0.0f;
		else if( t < a ) return std::pow( t / a, aExp );
		else if( t < a + d ) return std::pow( 1.0f - ( t - a ) / d, dExp ) * ( 1.0f - sLvl ) + sLvl;
		else if( t < a + d + s ) return sLvl;
		else if( t < a + d + s + r ) return std::pow( 1.0f - ( t - a - d - s ) / r, rExp ) * sLvl;
		else return 0.0f;
		} );
	}

} // namespace flan
