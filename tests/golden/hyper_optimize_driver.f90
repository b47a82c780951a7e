!  hyper_optimize_driver.f90 -- TEST INFRASTRUCTURE, not product code.
!
!  A bind(C) driver over the UNMODIFIED reference modules, compiled by tests/golden/make_hyper_optimize.py against the module files
!  and objects the oracle recipe leaves in oracle/_ref/obj_parity (same flags: -O2 -ffp-contract=off).  One entry, ho_run:
!    1  mw_optimize::optimize_hyper_lbfgsb (mw_optimize.f90:779-958) as it is: the final cost and the calibrated planes.  That routine
!       keeps its control vector, its bounds and its hyper matrices to itself, so
!    2  the same calibration once more, step by step, from this file: the module's own set-up routines -- private there, reached
!       through their link names -- give x0, l, u and nbd; lbfgsb.f's setulb is driven by its documented reverse-communication protocol
!       with the module's settings (m = 10, factr = 1e6, pgtol = 1e-12, the two stop tests), every evaluation is mw_forward::
!       hyper_forward_b; the cost of every iterate and the final hyper matrices are recorded.
!  The recorder only accepts 2 when its final cost and every mapped plane equal those of 1 bit for bit.
!
!  This file is ours; it contains no reference source text.  Nothing compiled from it is committed.

module hyper_optimize_driver

    use iso_c_binding
    use md_constant
    use mwd_setup
    use mwd_mesh
    use mwd_input_data
    use mwd_parameters
    use mwd_states
    use mwd_output
    use mwd_parameters_manipulation
    use mwd_states_manipulation
    use mw_forward, only: hyper_forward, hyper_forward_b
    use mw_optimize, only: optimize_hyper_lbfgsb

    implicit none

    !  the private set-up routines of mw_optimize under their link names; derived types travel by address
    interface
        subroutine ref_normalize_descriptor(setup, input_data, min_descriptor, max_descriptor) &
        & bind(C, name="_QMmw_optimizePnormalize_descriptor_hyper_lbfgsb")
            import :: c_float
            type(*) :: setup, input_data
            real(c_float) :: min_descriptor(*), max_descriptor(*)
        end subroutine ref_normalize_descriptor
        subroutine ref_problem_initialise(n, setup, mesh, parameters, states, hyper_parameters, hyper_states, nbd, l, u) &
        & bind(C, name="_QMmw_optimizePproblem_initialise_hyper_lbfgsb")
            import :: c_int, c_double
            integer(c_int) :: n
            type(*) :: setup, mesh, parameters, states, hyper_parameters, hyper_states
            integer(c_int) :: nbd(*)
            real(c_double) :: l(*), u(*)
        end subroutine ref_problem_initialise
        subroutine ref_var_to_control(n, setup, hyper_parameters, hyper_states, x) &
        & bind(C, name="_QMmw_optimizePvar_to_control_hyper_lbfgsb")
            import :: c_int, c_double
            integer(c_int) :: n
            type(*) :: setup, hyper_parameters, hyper_states
            real(c_double) :: x(*)
        end subroutine ref_var_to_control
        subroutine ref_control_to_var(n, setup, hyper_parameters, hyper_states, x) &
        & bind(C, name="_QMmw_optimizePcontrol_to_var_hyper_lbfgsb")
            import :: c_int, c_double
            integer(c_int) :: n
            type(*) :: setup, hyper_parameters, hyper_states
            real(c_double) :: x(*)
        end subroutine ref_control_to_var
    end interface

contains

    !  icfg = (structure 1..5; nrow; ncol; nt; ng; nd; mapping 1 linear, 2 polynomial; maxiter; n = flagged fields x nhyper; niter_cap)
    !  rcfg = (dt; dx)
    !  arrays column-major as the reference holds them, path and gauge_pos 1-based; params / states the (nrow, ncol, GNP / GNS) packings
    !  out: x0, l, u, nbd (n); costs(1) = the first evaluation's cost, costs(1 + i) = the cost at iterate i, niter = iterates completed;
    !  final_cost / hyper_p / hyper_s / params_out / states_out of the step-by-step run; ref_cost / ref_params / ref_states of
    !  optimize_hyper_lbfgsb itself; desc_norm = the normalised descriptors; desc_back = the descriptors as optimize_hyper_lbfgsb returns them
    subroutine ho_run(icfg, rcfg, flwdir, flwacc, path, active_cell, gauge_pos, area, prcp, pet, qobs, descriptor, params, states, &
    & optim_p, optim_s, x0, l, u, nbd, costs, niter, final_cost, hyper_p, hyper_s, params_out, states_out, &
    & ref_cost, ref_params, ref_states, desc_norm, desc_back) bind(C, name="ho_run")

        integer(c_int), intent(in) :: icfg(10)
        real(c_float), intent(in) :: rcfg(2)
        integer(c_int), intent(in) :: flwdir(icfg(2), icfg(3)), flwacc(icfg(2), icfg(3))
        integer(c_int), intent(in) :: path(2, icfg(2)*icfg(3)), active_cell(icfg(2), icfg(3))
        integer(c_int), intent(in) :: gauge_pos(icfg(5), 2)
        real(c_float), intent(in) :: area(icfg(5))
        real(c_float), intent(in) :: prcp(icfg(2), icfg(3), icfg(4)), pet(icfg(2), icfg(3), icfg(4))
        real(c_float), intent(in) :: qobs(icfg(5), icfg(4)), descriptor(icfg(2), icfg(3), icfg(6))
        real(c_float), intent(in) :: params(icfg(2), icfg(3), GNP), states(icfg(2), icfg(3), GNS)
        integer(c_int), intent(in) :: optim_p(GNP), optim_s(GNS)
        real(c_double), intent(inout) :: x0(icfg(9)), l(icfg(9)), u(icfg(9))
        integer(c_int), intent(inout) :: nbd(icfg(9))
        real(c_float), intent(inout) :: costs(icfg(10) + 1)
        integer(c_int), intent(inout) :: niter
        real(c_float), intent(inout) :: final_cost, ref_cost
        real(c_float), intent(inout) :: hyper_p(1 + icfg(7)*icfg(6), 1, GNP), hyper_s(1 + icfg(7)*icfg(6), 1, GNS)
        real(c_float), intent(inout) :: params_out(icfg(2), icfg(3), GNP), states_out(icfg(2), icfg(3), GNS)
        real(c_float), intent(inout) :: ref_params(icfg(2), icfg(3), GNP), ref_states(icfg(2), icfg(3), GNS)
        real(c_float), intent(inout) :: desc_norm(icfg(2), icfg(3), icfg(6)), desc_back(icfg(2), icfg(3), icfg(6))

        type(SetupDT) :: setup
        type(MeshDT) :: mesh
        type(Input_DataDT) :: input_data
        type(ParametersDT) :: p, p_b
        type(StatesDT) :: s, s_b
        type(OutputDT) :: output, output_b
        type(Hyper_ParametersDT) :: hp, hp_b, hp_bgd
        type(Hyper_StatesDT) :: hs, hs_b, hs_bgd
        integer :: nrow, ncol, nt, ng, nd, n, m, iprint, maxiter
        integer, allocatable :: iwa(:)
        real(dp), allocatable :: x(:), g(:), wa(:)
        real(dp) :: factr, pgtol, f
        character(lchar) :: task, csave
        logical :: lsave(4)
        integer :: isave(44)
        real(dp) :: dsave(29)
        real(sp) :: cost, cost_b
        real(sp) :: dmin(max(icfg(6), 1)), dmax(max(icfg(6), 1))
        external :: setulb

        nrow = icfg(2); ncol = icfg(3); nt = icfg(4); ng = icfg(5); nd = icfg(6); maxiter = icfg(8); n = icfg(9)
        select case (icfg(1))
        case (1); setup%structure = "gr-a"
        case (2); setup%structure = "gr-b"
        case (3); setup%structure = "gr-c"
        case (4); setup%structure = "gr-d"
        case (5); setup%structure = "vic-a"
        end select
        setup%dt = rcfg(1)
        setup%ntime_step = nt
        call SetupDT_initialise(setup, nd, ng)
        deallocate (setup%optimize%wgauge)
        if (icfg(7) .eq. 1) then
            call Optimize_SetupDT_initialise(setup%optimize, nt, nd, ng, "hyper-linear", 0, 0)
        else
            call Optimize_SetupDT_initialise(setup%optimize, nt, nd, ng, "hyper-polynomial", 0, 0)
        end if
        setup%optimize%verbose = .false.
        setup%optimize%denormalize_forward = .false.
        setup%optimize%optimize_start_step = 1
        setup%optimize%njf = 1
        setup%optimize%njr = 0
        deallocate (setup%optimize%jobs_fun, setup%optimize%wjobs_fun)
        allocate (setup%optimize%jobs_fun(1), setup%optimize%wjobs_fun(1))
        setup%optimize%jobs_fun(1) = "nse"
        setup%optimize%wjobs_fun(1) = 1._sp
        setup%optimize%wjreg = 0._sp
        setup%optimize%wgauge = 1._sp/real(ng, sp)
        setup%optimize%optim_parameters = optim_p
        setup%optimize%optim_states = optim_s
        setup%optimize%maxiter = maxiter

        call MeshDT_initialise(mesh, setup, nrow, ncol, ng)
        mesh%dx = rcfg(2)
        mesh%flwdir = flwdir
        mesh%flwacc = flwacc
        mesh%path = path
        mesh%active_cell = active_cell
        mesh%nac = count(active_cell .eq. 1)
        mesh%gauge_pos = gauge_pos
        mesh%area = area

        call Input_DataDT_initialise(input_data, setup, mesh)
        input_data%qobs = qobs
        input_data%prcp = prcp
        input_data%pet = pet
        input_data%descriptor = descriptor

        call ParametersDT_initialise(p, mesh)
        call ParametersDT_initialise(p_b, mesh)
        call StatesDT_initialise(s, mesh)
        call StatesDT_initialise(s_b, mesh)
        call OutputDT_initialise(output, setup, mesh)
        call OutputDT_initialise(output_b, setup, mesh)

        !  1  the reference's routine as it is
        call set_parameters(mesh, p, params)
        call set_states(mesh, s, states)
        call optimize_hyper_lbfgsb(setup, mesh, input_data, p, s, output)
        ref_cost = output%cost
        call get_parameters(mesh, p, ref_params)
        call get_states(mesh, s, ref_states)
        desc_back = input_data%descriptor

        !  2  step by step
        input_data%descriptor = descriptor
        call set_parameters(mesh, p, params)
        call set_states(mesh, s, states)
        call Hyper_ParametersDT_initialise(hp, setup)
        call Hyper_ParametersDT_initialise(hp_b, setup)
        call Hyper_StatesDT_initialise(hs, setup)
        call Hyper_StatesDT_initialise(hs_b, setup)
        call ref_normalize_descriptor(setup, input_data, dmin, dmax)
        desc_norm = input_data%descriptor

        m = 10
        factr = 1.e6_dp
        pgtol = 1.e-12_dp
        iprint = -1
        allocate (x(n), g(n), iwa(3*n), wa(2*m*n + 5*n + 11*m*m + 8*m))
        call ref_problem_initialise(n, setup, mesh, p, s, hp, hs, nbd, l, u)
        hp_bgd = hp
        hs_bgd = hs
        call ref_var_to_control(n, setup, hp, hs, x)
        x0 = x

        niter = 0
        costs = 0._sp
        task = 'START'
        do while (task(1:2) .eq. 'FG' .or. task .eq. 'NEW_X' .or. task .eq. 'START')
            call setulb(n, m, x, l, u, nbd, f, g, factr, pgtol, wa, iwa, task, iprint, csave, lsave, isave, dsave)
            call ref_control_to_var(n, setup, hp, hs, x)
            if (task(1:2) .eq. 'FG') then
                cost_b = 1._sp
                cost = 0._sp
                call hyper_forward_b(setup, mesh, input_data, p, p_b, hp, hp_b, hp_bgd, s, s_b, hs, hs_b, hs_bgd, output, output_b, &
                & cost, cost_b)
                f = real(cost, kind(f))
                call ref_var_to_control(n, setup, hp_b, hs_b, g)
                if (task(4:8) .eq. 'START') costs(1) = cost
            end if
            if (task(1:5) .eq. 'NEW_X') then
                niter = isave(30)
                if (niter .le. icfg(10)) costs(1 + niter) = real(f, sp)
                if (isave(30) .ge. maxiter) task = 'STOP: ITERATIONS'
                if (dsave(13) .le. 1.d-10*(1.0d0 + abs(f))) task = 'STOP: PROJECTED GRADIENT'
            end if
        end do

        call hyper_forward(setup, mesh, input_data, p, hp, hp_bgd, s, hs, hs_bgd, output, cost)
        final_cost = cost
        call hyper_parameters_to_parameters(hp, p, setup, mesh, input_data)
        call hyper_states_to_states(hs, s, setup, mesh, input_data)
        call get_hyper_parameters(setup, hp, hyper_p)
        call get_hyper_states(setup, hs, hyper_s)
        call get_parameters(mesh, p, params_out)
        call get_states(mesh, s, states_out)

    end subroutine ho_run

end module hyper_optimize_driver
